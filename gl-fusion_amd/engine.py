"""Caller-side harness with the reference Trainer's surface (main.py:63-883) for the hot path:
`Trainer(config)`, `.train(is_backbone, is_cycle)`, `.eval(net_path, is_fuse, raw_data)`,
`.test_visualize(method_name, net_path)`, `_calculate_overlap_metrics`, `save()`, `load()`.  With config['train']['infos'] / ['video_infos'] the Trainer trains from
patient volumes: data.BatchLoader over per-view SegPAHDatasets for the supervised batches (main.py:116-117, 139) and
data.ClipLoader over AlignedVideoSegPAHDatasets for the cycle term's clips (main.py:119-122, 143-145), the volumes resident
on the device (data.VolumeStore).  The reference's NIfTI files are not shipped (absolute paths on the authors' machine, SURVEY
section 0), so without those keys the loaders produce synthetic clips with the same tensor contract: images [N,1,112,112]
in [0,1], masks [N,5,112,112] in {0,1} (datasets/loader.py:298-330); the unlabelled "video" loader of the cycle term yields
clips of `clip_length` frames per view (main.py:213-218).  `is_cycle=True` adds the temporal cycle-consistency loss of main.py:213-237
(second forward on the video clip, pooled global-fusion features, seg_cycle / dense_seg_cycle, total = seg + 1e-2 cyc).
config['net']['model'] names any of MODELS -- Global_and_Local, its nine variants of models/ours.py and the five baselines; OUTPUTS says
where each model's output tuple carries what the Trainer uses.  config['train']['cps_weight'] > 0 adds the cross pseudo supervision
term of Global_and_Local_CPS on the same clip forward (ops.cps_bce_sum).
"""
from __future__ import annotations

import functools
import glob
import os
import warnings
from collections import namedtuple
from typing import Dict, Iterator, Tuple

import torch

from . import ops
from .ddp import GradAllReducer, all_reduce_counts, default_ignore
from .optim import SGD, Adam
from . import models as _models
from .models import Global_and_Local, MLP_fusion, baseline_unet, early_fusion, late_fusion, multiview_unet

# config['net']['model'] -> class; the U-Net baselines return (mask, None, None, x5) and the fusion baselines (mask, f4, None, None):
# no backbone mask, no fusion features
MODELS = {"Global_and_Local": Global_and_Local, "baseline_unet": baseline_unet, "multiview_unet": multiview_unet,
          "early_fusion": early_fusion, "late_fusion": late_fusion, "MLP_fusion": MLP_fusion}
NO_FUSION_FEATURES = ("baseline_unet", "multiview_unet", "early_fusion", "late_fusion", "MLP_fusion")
# the ablation variants of models/ours.py
VARIANTS = ("Global_and_Local_cyc_nofusion", "Foreground_and_Background", "Global_and_Local_Temporal", "Global_and_Local_conv_merge",
            "Global_only", "Global_only_cyc_nofusion", "Local_only", "model19", "Global_and_Local_CPS")
MODELS.update({name: getattr(_models, name) for name in VARIANTS})

# Where each model's output tuple carries what the Trainer uses -- every method reads the tuple through this table:
#   heads     outputs supervised by the BCE sum; the first is the one scored (epoch Dice, eval, validation, pictures)
#   backbone  the output a scoring pass takes with is_fuse=False (None: the model has no second mask, the first head is scored)
#   cycle     the output whose (h, w)-pooled features feed the cycle term (None: no fusion features, no cycle term)
#   clip_is_video  the forward takes is_video: True for the unlabelled clip (one video), False for a labelled batch
# Local_only: out[2] is the detached [N,1,h,w] gate map -- the reference's sum(dim=(2, 3)) of it is ONE feature without a gradient, a
# cycle term that can move nothing -- so this ablation's cycle term acts on out[3], the local-fusion features.
# Global_and_Local_CPS: two networks, both masks supervised; with is_fuse=False network 2's mask is scored; the cycle features are
# network 1's.
Outputs = namedtuple("Outputs", "heads backbone cycle clip_is_video")
_MAIN = Outputs(heads=(0,), backbone=1, cycle=2, clip_is_video=False)
OUTPUTS = {name: _MAIN for name in ("Global_and_Local", "Global_and_Local_cyc_nofusion", "Global_and_Local_conv_merge",
                                    "Foreground_and_Background", "Global_only", "Global_only_cyc_nofusion", "model19")}
OUTPUTS["Global_and_Local_Temporal"] = _MAIN._replace(clip_is_video=True)
OUTPUTS["Local_only"] = _MAIN._replace(cycle=3)
OUTPUTS["Global_and_Local_CPS"] = _MAIN._replace(heads=(0, 1))
OUTPUTS.update({name: Outputs(heads=(0,), backbone=None, cycle=None, clip_is_video=False) for name in NO_FUSION_FEATURES})


def _cps_ignore(name: str) -> bool:
    if name.startswith("network."):
        return not name.startswith("network.backbone.")
    return default_ignore(name)


def reducer_ignore(model_name: str):
    """The `ignore` predicate GradAllReducer gets for a model: ddp.default_ignore, which drops the dead `network.*` template -- except for
    Global_and_Local_CPS, whose network 2 runs ON the template's encoders (models/ours.py: the `_2` ModuleDicts alias
    `network.backbone.*`, the name their parameters are listed under): those are reduced, `network.classifier.*` stays dead."""
    return _cps_ignore if model_name == "Global_and_Local_CPS" else default_ignore


class SyntheticClips:
    """Per-view iterator of (img, mask) batches on the device, deterministic per (seed, rank)."""

    def __init__(self, views, frames: int, h: int, w: int, device, seed: int = 1234, length: int = 8):
        self.views, self.frames, self.h, self.w, self.device, self.length = list(views), frames, h, w, device, length
        self.gen = torch.Generator(device=device).manual_seed(seed)

    def __len__(self) -> int:
        return self.length

    def batch(self) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
        imgs = {v: torch.rand(self.frames, 1, self.h, self.w, device=self.device, generator=self.gen) for v in self.views}
        masks = {v: (torch.rand(self.frames, 5, self.h, self.w, device=self.device, generator=self.gen) < 0.3).float() for v in self.views}
        return imgs, masks

    def __iter__(self) -> Iterator:
        for _ in range(self.length):
            yield self.batch()


class StepGraph:
    """One training step -- forward, loss, backward of a FIXED-shape batch -- recorded once as a hipGraph and replayed.

    The eager step issues ~3 200 kernel launches from Python (autograd Functions + ctypes), ~230 ms of host work per 264 ms
    step at config 2: the launch thread, not the GPU, bounds any further speed-up.  A replay costs one hipGraphLaunch.

        graph = StepGraph(step_fn, params)      # step_fn(): zero-arg closure over STATIC input tensors; returns the loss
        loss = graph.replay()                   # every kernel of the step runs again; loss / .grad tensors are static

    What makes the step capture-safe (none of it changes results):
      * weight-derived images are rebuilt by ops.refresh_weights() INSIDE the captured work (static buffers, four launches),
        so a replay after an optimizer step sees the new parameters;
      * Dropout masks depend on a device step counter the captured work advances first thing (ops.advance_step);
      * the slot pools of operand maxima / BatchNorm sums are re-created inside the capture (their zero fill is replayed);
      * the independent sections of a forward use pairwise different side streams (ops.SECTIONS_DISTINCT; re-using one side
        stream in two fork/join groups of a capture crashes hipStreamEndCapture on ROCm 7.2);
      * nothing in the step synchronises the host or allocates outside torch's allocator.
    Gradient all-reduce stays OUTSIDE the graph (GradAllReducer in deferred mode: the hooks' bucket copies are captured, the
    collectives are launched by finalize() after each replay).
    Update parameters only in place (the fused Adam does): the graph holds their addresses."""

    def __init__(self, step_fn, params, warmup: int = 2, reducer=None, refresh_weights: bool = True):
        self.params = [p for p in params]
        if not self.params:
            raise RuntimeError("StepGraph: no parameters")
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("StepGraph needs CUDA(HIP) parameters: the engine has no CPU fallback")
        self.device = dev
        self.reducer = reducer
        if reducer is not None:
            reducer.deferred = True
        prev_distinct, ops.SECTIONS_DISTINCT = ops.SECTIONS_DISTINCT, True
        self._prev_distinct = prev_distinct

        self.wtable = None                         # frozen job table of THIS model's weight images (made after the warm-up)

        def body():
            ops.advance_step(dev)
            if refresh_weights:
                ops.refresh_weights(self.wtable)   # warm-up: the registry-wide refresh; captured: this model's images only
            for p in self.params:
                p.grad = None
            return step_fn()

        self.stream = torch.cuda.Stream(device=dev)            # warm-up and capture share it (library rings, pools, allocator)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        try:
            with torch.cuda.stream(self.stream):
                for _ in range(max(1, warmup)):                    # lazily-created state (caches, job table, rings) settles here
                    out = body()
                    if reducer is not None:
                        reducer.finalize()
                del out
                torch.cuda.synchronize(dev)
                for p in self.params:
                    p.grad = None
                ops.reset_capture_pools()
                if refresh_weights:
                    # the captured refresh replays against a table of its own: it names only this model's images and keeps their
                    # buffers alive, so nothing another model (or the garbage collector) does to the registry can invalidate it
                    self.wtable = ops.freeze_weight_table(self.params)
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, stream=self.stream):
                    self.out = body()
        except BaseException:
            # a failed warm-up / capture must not leave the process in capture configuration: the reducer back to
            # immediate mode, the section stream policy back to what it was
            if reducer is not None:
                reducer.deferred = False
            ops.SECTIONS_DISTINCT = prev_distinct
            raise
        torch.cuda.current_stream(dev).wait_stream(self.stream)
        self.grads = {p: p.grad for p in self.params if p.grad is not None}      # static tensors the replays write

    def replay(self):
        """Run the recorded step on the current stream.  Returns step_fn()'s (static) result."""
        self.graph.replay()
        ops.stats_moved()                            # a recorded training step moves running statistics without Python seeing it
        if self.reducer is not None and self.reducer.world > 1:
            self.reducer.finalize()                  # re-points .grad at the reduced bucket slices
        else:
            for p, g in self.grads.items():          # an optimizer's zero_grad(set_to_none=True) may have dropped them
                p.grad = g
        return self.out

    def release(self) -> None:
        """Free the graph and its private memory pool."""
        ops.SECTIONS_DISTINCT = self._prev_distinct
        if self.reducer is not None:
            self.reducer.deferred = False
        self.graph = None
        self.out = None
        self.grads = {}
        self.wtable = None


def _contour_line(rep: dict) -> str:
    """One printed line of a view's contour report (data.ContourAccumulator.report): pixels; '-' where no pair was scored."""
    def fmt(x):
        return "-" if x is None else f"{x:.3f}"
    mean = rep["mean"] or (None, None, None)
    return (f"contour (pixels) hd {fmt(mean[0])} hd95 {fmt(mean[1])} assd {fmt(mean[2])}; part hd " + " ".join(fmt(x) for x in rep["hd"])
            + "; part hd95 " + " ".join(fmt(x) for x in rep["hd95"]) + "; part assd " + " ".join(fmt(x) for x in rep["assd"])
            + "; pairs scored/missed/spurious/absent "
            + " ".join(f"{a}/{b}/{c}/{d}" for a, b, c, d in zip(rep["scored"], rep["missed"], rep["spurious"], rep["absent"])))


def _fold_bn_scope(fn):
    """Run a Trainer method with ops.set_fold_bn(True) / ops.set_fold_bn_s16(True) when config['train']['fold_bn'] /
    config['train']['fold_bn_s16'] ask for it; the previous values come back."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        prev, prev16 = ops.fold_bn(), ops.fold_bn_s16()
        if self.fold_bn:
            ops.set_fold_bn(True)
        if self.fold_bn_s16:
            ops.set_fold_bn_s16(True)
        try:
            return fn(self, *args, **kwargs)
        finally:
            ops.set_fold_bn(prev)
            ops.set_fold_bn_s16(prev16)
    return wrapped


class Trainer:
    def __init__(self, config: dict):
        self.config = config
        tr = config["train"]
        self.view_num = tr["view_num"]
        self.test_view = tr.get("test_view", self.view_num)
        self.device = tr.get("device", torch.device("cuda", 0))
        if not torch.cuda.is_available():
            raise RuntimeError("glfusion_amd.engine.Trainer needs an MI355X: the HIP engine has no CPU fallback")
        self.print_val = tr.get("global_rank", 0) == 0                       # main.py:92
        self.contour_metrics = bool(tr.get("contour_metrics", False))       # eval passes also report HD / HD95 / ASSD (not in the reference)
        # config['train']['precision'] (no reference counterpart): "f32" | "bf16x6" | "f16x3" | "f16" | "bf16" (16-bit activation storage,
        # BASELINE.json configs[2] / [4]); absent = whatever glfusion_amd.ops is set to
        if tr.get("precision"):
            ops.set_precision(tr["precision"])
        # config['train']['fold_bn'] (absent = False): eval() and validation_and_test() run with BatchNorm folded into the convolutions
        # (ops.set_fold_bn; takes effect under "f16x3" / "f16" only, training is never touched)
        self.fold_bn = bool(tr.get("fold_bn", False))
        # config['train']['fold_bn_s16'] (absent = False): the same for 16-bit storage (ops.set_fold_bn_s16; takes effect under "bf16" only)
        self.fold_bn_s16 = bool(tr.get("fold_bn_s16", False))
        # config['net']['model'] (absent = "Global_and_Local", main.py:150): which of MODELS the Trainer builds
        self.model_name = config["net"].get("model", "Global_and_Local")
        if self.model_name not in MODELS:
            raise ValueError(f"glfusion_amd: config['net']['model'] = {self.model_name!r}; the Trainer builds one of {sorted(MODELS)}")
        self.outputs = OUTPUTS[self.model_name]
        # config['train']['cps_weight'] (absent = 0; no reference counterpart): weight of the cross pseudo supervision term of
        # Global_and_Local_CPS -- on an unlabelled clip each network's hard prediction supervises the other (ops.cps_bce_sum)
        self.cps_weight = float(tr.get("cps_weight", 0) or 0)
        if self.cps_weight < 0 or self.cps_weight != self.cps_weight:
            raise ValueError(f"glfusion_amd: config['train']['cps_weight'] = {self.cps_weight!r} must be >= 0")
        if self.cps_weight > 0 and self.model_name != "Global_and_Local_CPS":
            raise ValueError(f"glfusion_amd: config['train']['cps_weight'] = {self.cps_weight!r} needs the two networks of "
                             f"Global_and_Local_CPS; {self.model_name} has one")
        self.cps_report = {}                                                    # {view: agreement fraction of the two networks}, per epoch
        self._cps_stats = None                                                  # {view: int64[4]} the last CPS step filled
        self.clip_cycle = True                                                  # a train_step with a clip adds the cycle term (train() sets it)
        self.model = MODELS[self.model_name](view_num=self.view_num).to(self.device)
        opt = config["net"]["opt"]
        name = opt.get("opt_name", "Adam")
        if name == "SGD":
            # main.py:159-161 (plain SGD), fused; opt['momentum'] / opt['dampening'] / opt['nesterov'] have no reference counterpart, absent = off
            self.optimizer = SGD(self.model.parameters(), lr=opt["lr"], weight_decay=opt["weight_decay"], momentum=opt.get("momentum", 0),
                                 dampening=opt.get("dampening", 0), nesterov=bool(opt.get("nesterov", False)))
        elif name == "Adam":
            self.optimizer = Adam(self.model.parameters(), lr=opt["lr"], weight_decay=opt["weight_decay"])    # main.py:162-165, fused
        else:
            raise ValueError(f"glfusion_amd: config['net']['opt']['opt_name'] = {name!r}; main.py:158-165 has the branches 'SGD' and 'Adam'")
        # config['train']['clip_grad_norm'] (absent = off): every step clips by this global gradient norm and skips itself when the
        # norm is not finite, all on the device (optim._Fused.set_grad_clip).  The optimizer step is outside a recorded graph and
        # behind reducer.finalize(), so the eager, cycle and graph-replayed steps and every rank see the same (reduced) norm.
        self.clip_grad_norm = tr.get("clip_grad_norm")
        if self.clip_grad_norm is not None:
            self.optimizer.set_grad_clip(float(self.clip_grad_norm))
        self.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=tr["num_epochs"])   # main.py:168
        # config['train']['save_optimizer'] (absent = False): save() also writes opt_%05d.pth, the file load() resumes the optimizer from
        self.save_optimizer = bool(tr.get("save_optimizer", False))
        self.latest_epoch = 0                                                   # first epoch train() runs; load() moves it
        if tr.get("is_load", False):                                            # main.py:74, 153
            self.load()
        self.reducer = GradAllReducer(self.model, ignore=reducer_ignore(self.model_name))
        self.reducer.broadcast_parameters(0)
        frames = tr["batch_size"] * tr.get("frames_per_clip", 1)
        self.dense_cyc = bool(tr.get("dense_cyc", False))                      # main.py:228
        # config['train']['graph']: replay the (cycle-free) training step from one hipGraph instead of issuing ~3 400 launches
        self.use_graph = bool(tr.get("graph", False))
        self._graph = None
        # config['train']['infos'] / ['video_infos'] (dicts, or paths to the reference's .npy, main.py:283): train from patient
        # volumes -- the supervised batches of main.py:116-117, 139 and the cycle term's clips of main.py:119-122, 143-145, over
        # config['train']['train_list'] (the reference's data_list/train_list.npy; absent = the datasets' own split) and
        # config['train']['use_data'] (set_select), the volumes resident on the device within config['train']['store_bytes'].
        # Absent: that loader is synthetic, as before.
        self.loader = self.video_loader = None
        if tr.get("infos") is not None or tr.get("video_infos") is not None:
            from . import data as _data
            import torch.distributed as dist
            rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_initialized() else (0, 1)
            self.store = _data.VolumeStore(self.device, int(tr.get("store_bytes", 8 << 30)))
            common = dict(is_train=True, data_list=tr.get("train_list"), set_select=tuple(tr.get("use_data", ("rmyy",))))
            if tr.get("infos") is not None:
                infos = _data.load_infos(tr["infos"])
                self.loader = _data.BatchLoader({v: _data.SegPAHDataset(infos, view_num=[v], single_frame=True, device=self.device,
                                                                        seg_parts=bool(tr.get("seg_parts", True)), **common)
                                                 for v in self.view_num}, tr["batch_size"], self.store, rank, world)
            if tr.get("video_infos") is not None:
                # main.py:136 and 191 iterate `train_cyc_dataset`, a dict the reference never fills; the clips it means are
                # train_pseudo_dataset's (main.py:119-122): Aligned_Video_Seg_PAHDataset over the whole-video infos
                infos = _data.load_infos(tr["video_infos"])
                self.video_loader = _data.ClipLoader({v: _data.AlignedVideoSegPAHDataset(infos, view_num=[v], random_sample=False,
                                                                                         clip_length=int(tr.get("clip_length", 40)), **common)
                                                      for v in self.view_num}, self.store, rank, world)
        if self.loader is None:
            self.loader = SyntheticClips(self.view_num, frames, 112, 112, self.device, seed=1234 + tr.get("global_rank", 0),
                                         length=tr.get("iters_per_epoch", 4))
        if self.video_loader is None:
            self.video_loader = SyntheticClips(self.view_num, int(tr.get("clip_length", 40)), 112, 112, self.device,
                                               seed=4321 + tr.get("global_rank", 0), length=tr.get("iters_per_epoch", 4))

    def cycle_loss(self, video: Dict[str, torch.Tensor]) -> torch.Tensor:
        """main.py:213-235: second forward on an unlabelled clip [T,1,H,W] per view, global-fusion features summed
        over (h, w), seg_cycle (or dense_seg_cycle) per view with target_region 16, cyc_off 2, chunk_size 3,
        temperature 10."""
        self._require_fusion_features("cycle_loss")
        return self._clip_terms(video, cycle=True, cps=False)[0]

    def _forward(self, x, clip: bool = False):
        """The model's forward on a labelled batch, or (clip) on an unlabelled clip -- one video, which Global_and_Local_Temporal
        is told (OUTPUTS[...].clip_is_video)."""
        return self.model(x, is_video=clip) if self.outputs.clip_is_video else self.model(x)

    def _clip_terms(self, video: Dict[str, torch.Tensor], cycle: bool, cps: bool):
        """ONE forward on the unlabelled clip for both terms that use it: (cycle loss, CPS loss), None for a term not asked for.
        The cycle term takes the model's cycle features (OUTPUTS: out[2]; Local_only out[3], the local-fusion features, because its
        out[2] is the detached gate map); the CPS term sum_{v in test_view} ops.cps_bce_sum of the two networks' masks, whose
        agreement counts stay in self._cps_stats."""
        out = self._forward(video, clip=True)
        cyc = cross = None
        if cycle:
            feats = ops.pooled_fusion_features(out[self.outputs.cycle])
            for view in self.view_num:
                if self.dense_cyc:
                    l = ops.dense_seg_cycle(feats[view], 16, 2, 3, 10, soft_label=False, is_overlap=True)
                else:
                    l = ops.seg_cycle(feats[view], 16, 2, 3, 10)
                cyc = l if cyc is None else cyc + l
        if cps:
            if self._cps_stats is None:
                self._cps_stats = {v: torch.empty(4, dtype=torch.int64, device=self.device) for v in self.test_view}
            h1, h2 = self.outputs.heads
            for view in self.test_view:
                l = ops.cps_bce_sum(out[h1][view], out[h2][view], self._cps_stats[view])
                cross = l if cross is None else cross + l
        return cyc, cross

    def _supervised_loss(self, out, masks):
        """sum over the model's supervised heads and the views of test_view of the BCE sum (main.py:209-211; CPS: both networks)."""
        loss = None
        for head in self.outputs.heads:
            for view in self.test_view:
                l = ops.bce_with_logits_sum(out[head][view], masks[view])
                loss = l if loss is None else loss + l
        return loss

    def _graph_step(self, imgs, masks):
        """The segmentation step (no cycle term) replayed from ONE hipGraph (StepGraph): the batch is copied into static input
        buffers, the recorded forward + loss + backward (+ weight-image refresh) runs, the optimizer updates the parameters in place.
        The optimizer step is NOT part of the recorded work, so either optimizer (fused Adam or fused SGD) runs behind the same graph:
        both write the parameters through their existing addresses, and their state lives outside the graph's memory pool.
        Recorded at the first call; the batch shape must not change afterwards."""
        if self._graph is None:
            self._static = ({v: torch.empty_like(t) for v, t in imgs.items()}, {v: torch.empty_like(t) for v, t in masks.items()})
            s_imgs, s_masks = self._static
            holder = {}

            def core():
                out = self._forward(s_imgs)
                holder["pred"] = out[self.outputs.heads[0]]
                loss = self._supervised_loss(out, s_masks)
                loss.backward()
                return loss.detach()
            for v in imgs:
                s_imgs[v].copy_(imgs[v]); s_masks[v].copy_(masks[v])
            self._graph = StepGraph(core, [p for p in self.model.parameters()], warmup=1, reducer=self.reducer if self.reducer.world > 1 else None)
            self._graph_pred = holder["pred"]
        s_imgs, s_masks = self._static
        for v in imgs:
            if imgs[v].shape != s_imgs[v].shape:
                raise RuntimeError("glfusion_amd.engine: a graph-replayed step needs batches of one shape (config['train']['graph'] = False for ragged ones)")
            s_imgs[v].copy_(imgs[v]); s_masks[v].copy_(masks[v])
        loss = self._graph.replay()
        self.optimizer.step()
        return loss, self._graph_pred

    def train_step(self, imgs, masks, video=None) -> torch.Tensor:
        """main.py:202-243: forward, sum over heads and views of the BCE-sum, backward, optimizer step.  With an unlabelled clip
        `video`, ONE forward on it adds cps_weight x the CPS term (config['train']['cps_weight'] > 0) and, unless self.clip_cycle
        is False (train(is_cycle=False) draws its clip for the CPS term alone), 1e-2 x the cycle loss (main.py:237).  Returns (loss,
        the first head's masks)."""
        cycle = self.clip_cycle
        if video is None and self.use_graph:
            return self._graph_step(imgs, masks)
        out = self._forward(imgs)
        loss = self._supervised_loss(out, masks)
        if video is not None:
            if cycle:
                self._require_fusion_features("train_step with a clip")
            cyc, cross = self._clip_terms(video, cycle=cycle, cps=self.cps_weight > 0)
            if cross is not None:
                loss = loss + self.cps_weight * cross
            if cyc is not None:
                loss = loss + 1e-2 * cyc                                       # main.py:237
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.reducer.finalize()
        self.optimizer.step()
        return loss.detach(), out[self.outputs.heads[0]]

    def _prediction(self, out, is_fuse: bool):
        """The mask a scoring pass takes from the model's outputs (OUTPUTS): the first head, or with is_fuse False the model's second
        mask -- the backbone mask out[1]; for Global_and_Local_CPS network 2's -- where the model has one.  The U-Net baselines
        return None there and the fusion baselines their layer-4 features: their one mask is scored whatever is_fuse says."""
        if is_fuse or self.outputs.backbone is None:
            return out[self.outputs.heads[0]]
        return out[self.outputs.backbone]

    def _require_fusion_features(self, what: str) -> None:
        if self.outputs.cycle is None:
            raise ValueError(f"glfusion_amd: {what} needs the model's fusion features (its third output), and {self.model_name} "
                             "returns none: train it with is_cycle=False")

    def train(self, is_backbone: bool = False, is_cycle: bool = True):
        if is_cycle:
            self._require_fusion_features("Trainer.train(is_cycle=True)")
        use_clip = is_cycle or self.cps_weight > 0              # the CPS term draws a clip too, with or without the cycle term
        if use_clip and not isinstance(self.loader, SyntheticClips) and isinstance(self.video_loader, SyntheticClips):
            what, without = (("Trainer.train(is_cycle=True)", "is_cycle=False") if is_cycle else
                             ("config['train']['cps_weight'] > 0", "cps_weight 0"))
            raise ValueError(f"glfusion_amd: {what} with config['train']['infos'] needs config['train']['video_infos'] "
                             f"too: the clip terms would otherwise run on synthetic noise clips beside real batches ({without} trains without them)")
        self.clip_cycle = bool(is_cycle)
        try:
            self._train_epochs(use_clip)
        finally:
            self.clip_cycle = True

    def _train_epochs(self, use_clip: bool):
        # both kinds of loader serve one interface: iteration yields (imgs, masks) batches, batch()[0] is the next clip per view
        for epoch in range(self.latest_epoch, self.config["train"]["num_epochs"]):
            self.model.train()
            for imgs, masks in self.loader:
                video = self.video_loader.batch()[0] if use_clip else None
                loss, pred = self.train_step(imgs, masks, video)
            self.scheduler.step()
            # the epoch's Dice sums its counters over ranks: a collective, so EVERY rank computes it (only rank 0 prints)
            dice = {v: self._calculate_overlap_metrics(masks[v], pred[v].detach())[1] for v in self.test_view}
            if self.print_val:
                clip = ""
                if self.clip_grad_norm is not None:      # the epoch's one read of the device values, beside float(loss)
                    clip = f" grad-norm {float(self.optimizer.grad_norm):.4g} skipped-steps {int(self.optimizer.skipped_steps)}"
                if self.cps_weight > 0 and self._cps_stats is not None:
                    # the last step's agreement counts of the two networks, (n11 + n00) / numel per view: one host read per epoch
                    rows = torch.stack([self._cps_stats[v] for v in self.test_view]).tolist()
                    self.cps_report = {v: (r[0] + r[3]) / max(sum(r), 1) for v, r in zip(self.test_view, rows)}
                    clip += " cps-agreement " + " ".join(f"{v}:{a:.4f}" for v, a in self.cps_report.items())
                print(f"epoch {epoch}: loss {float(loss):.2f}{clip} dice {dice}")
                if self.config["train"].get("validate_every_epoch", True):
                    # main.py:259-274: validation runs on the printing rank alone, over every clip of the splits, with NO collective
                    # (the other ranks have already moved on to the next epoch's gradient all-reduces and wait there)
                    self.validation_and_test(net_root=None, is_fuse=True, raw_data=True, reduce=False)
            self.save(epoch)

    @torch.no_grad()
    @_fold_bn_scope
    def eval(self, net_path: str = None, is_fuse: bool = True, raw_data: bool = True, patients=None, on_clip=None):
        """main.py:417-543.  Per patient and view a raw clip volume goes through the data path (data.prepare_frames: the
        loader's resize / centre crop / part masks / 255 and the `[1,1,H,W,T] -> [T,1,H,W]` reshape of main.py:495-499),
        the model predicts all frames of the clip (the fused mask, or the backbone mask when is_fuse is False, main.py:
        504-506), BCE-sum losses accumulate per view (main.py:510-512) and the overlap counters accumulate over patients
        -- tp / fp / fn / tn are additive, so the reference's concatenation of every prediction (main.py:514-516) is not
        needed.  Returns {view: (pixel_acc, dice, precision, specificity, recall)} (main.py:519); the per-part Dice of
        main.py:537-543 and the losses are left in `self.eval_report`.  With config['train']['contour_metrics'] the report also
        holds 'contour' = {view: data.ContourAccumulator's report}: Hausdorff, 95th-percentile Hausdorff and average symmetric
        surface distance in pixels, averaged per part and per view over the (frame, part) pairs where both contours exist, and the
        counts of scored / missed / spurious / absent pairs; one launch per (patient, view), one collective and one host read per
        pass.  on_clip(k, view, logits, masks), if given, sees the device tensors of each (patient, view) this rank scores."""
        from .data import ContourAccumulator, SyntheticPatients, part_overlap_counts
        from . import data as _data
        if net_path and os.path.exists(net_path):
            self.model.load_state_dict(torch.load(net_path, map_location=self.device)["network"], strict=True)
        self.model.eval()
        if patients is None:
            patients = SyntheticPatients(self.view_num, int(self.config["train"].get("eval_patients", 2)),
                                         int(self.config["train"].get("clip_length", 40)), device=self.device, seed=77)
        counts = {v: torch.zeros(5, 4, dtype=torch.int64, device=self.device) for v in self.test_view}
        loss4view = {v: 0.0 for v in self.test_view}
        contour = {v: ContourAccumulator(5, self.device) for v in self.test_view} if self.contour_metrics else None
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_initialized() else 1
        rank = dist.get_rank() if dist.is_initialized() else 0
        for k, sample in enumerate(patients):
            if k % world != rank:                               # every rank scores its own share; counters and losses are summed below
                continue
            imgs, masks = {}, {}
            for v in self.view_num:
                imgs[v], masks[v] = _data.prepare_frames(sample[v][0], sample[v][1], v, train=False)
            out = self._forward(imgs)
            pred = self._prediction(out, is_fuse)
            for v in self.test_view:
                if on_clip is not None:
                    on_clip(k, v, pred[v], masks[v])
                counts[v] += part_overlap_counts(pred[v], masks[v])
                loss4view[v] += float(ops.bce_with_logits_sum(pred[v], masks[v]))
                if contour is not None:
                    contour[v] += (pred[v], masks[v])
        result, part_dice = {}, {}
        if world > 1:
            lt = torch.tensor([loss4view[v] for v in self.test_view], dtype=torch.float64, device=self.device)
            dist.all_reduce(lt)
            loss4view = {v: float(x) for v, x in zip(self.test_view, lt.tolist())}
        for v in self.test_view:
            per_part = all_reduce_counts(counts[v])
            result[v] = ops.overlap_metrics_from_counts(per_part.sum(dim=0))
            part_dice[v] = [ops.overlap_metrics_from_counts(per_part[c])[1] for c in range(5)]
        self.eval_report = {"loss": loss4view, "part_dice": part_dice}
        if contour is not None:
            self.eval_report["contour"] = ContourAccumulator.reports(contour, reduce=True)
        if self.print_val:
            for v in self.test_view:
                print(f"validation view {v}: loss {loss4view[v]:.4f} pixel-acc {result[v][0]:.4f} dice {result[v][1]:.4f} "
                      f"precision {result[v][2]:.4f} specificity {result[v][3]:.4f} recall {result[v][4]:.4f}; part dice "
                      + " ".join(f"{d:.4f}" for d in part_dice[v]))
                if contour is not None:
                    print(f"validation view {v}: " + _contour_line(self.eval_report["contour"][v]))
        return result

    @torch.no_grad()
    @_fold_bn_scope
    def test_visualize(self, method_name: str, net_path: str = None, out_root: str = "./visualze_for_ppt", patients=None,
                       is_fuse: bool = True, overlay_alpha=96, nifti: bool = True, on_clip=None):
        """main.py:546-648.  The data path of eval(): `patients` yields {view: (image volume, label volume)} (default: the
        synthetic patients eval() scores), patient k has the id '0_<k>', every clip goes through data.prepare_frames(train=False)
        and the model in eval mode (the fused mask, or the backbone mask when is_fuse is False).  Per patient and view of
        `test_view`, under <out_root>/<method_name>/192_data/<id>/<view>/ (the reference's directory and file name): pred_<frame>.png,
        the label map of main.py:606-609 in the colours of main.py:623-634; gnd_<frame>.png, the same rendering of the masks (the
        `visual_gnd` the reference computes and never saves); overlay_<frame>.png, the prediction laid over the grey frame with
        opacity overlay_alpha / 255 (None: not written; not in the reference).  With `nifti`, <out_root>/<method_name>/nifti/<id>/
        view<view>_pred.nii.gz holds the predicted class ids uint8 [H0,W0,T] in the geometry of the source volume
        (data.restore_labels), to be opened next to it.  The pictures are the model's own H x W pixels, one per prediction: the
        reference's dpi-600 matplotlib upscaling is not reproduced.  Rendering, colouring, blending and the back-projection are
        kernels; each output crosses to the host once per (patient, view).  on_clip(patient_id, view, logits, masks), if given,
        sees the device tensors of each (patient, view) before they are rendered.  Only the printing rank runs the pass; there is
        no collective in it.  Returns (and keeps as `self.visual_report`) {id: {view: {'png_dir', 'nifti' (path or None), 'frames'}}}."""
        from . import data as _data
        from . import nifti as _nifti
        from . import png as _png
        self.visual_report = manifest = {}
        if not self.print_val:
            return manifest
        if net_path and os.path.exists(net_path):
            self.model.load_state_dict(torch.load(net_path, map_location=self.device)["network"], strict=True)
        self.model.eval()
        if patients is None:
            patients = _data.SyntheticPatients(self.view_num, int(self.config["train"].get("eval_patients", 2)),
                                               int(self.config["train"].get("clip_length", 40)), device=self.device, seed=77)
        root = os.path.join(out_root, method_name)
        for k, sample in enumerate(patients):
            pid = f"0_{k}"
            imgs, masks = {}, {}
            for v in self.view_num:
                imgs[v], masks[v] = _data.prepare_frames(sample[v][0], sample[v][1], v, train=False)
            out = self._forward(imgs)
            pred = self._prediction(out, is_fuse)
            manifest[pid] = {}
            for v in self.test_view:
                if on_clip is not None:
                    on_clip(pid, v, pred[v], masks[v])
                pictures = {"pred": _data.render_labels(pred[v])[1], "gnd": _data.render_labels(masks[v])[1]}
                if overlay_alpha is not None:
                    pictures["overlay"] = _data.render_labels(pred[v], frames=imgs[v], alpha=overlay_alpha)[1]
                png_dir = os.path.join(root, "192_data", pid, v)
                os.makedirs(png_dir, exist_ok=True)
                for kind, rgba in pictures.items():
                    for frame_i, picture in enumerate(rgba.cpu().numpy()):       # one copy per (patient, view) and output
                        _png.write_rgba(os.path.join(png_dir, f"{kind}_{frame_i}.png"), picture)
                nii = None
                if nifti:
                    os.makedirs(os.path.join(root, "nifti", pid), exist_ok=True)
                    nii = os.path.join(root, "nifti", pid, f"view{v}_pred.nii.gz")
                    _nifti.write(nii, _data.restore_labels(pred[v], v, sample[v][0].shape).cpu().numpy())
                manifest[pid][v] = {"png_dir": png_dir, "nifti": nii, "frames": int(pred[v].shape[0])}
            print(f"patient {pid} pred finished")                                 # main.py:648
        return manifest

    @torch.no_grad()
    @_fold_bn_scope
    def validation_and_test(self, net_root: str = None, is_fuse: bool = True, raw_data: bool = True, infos: dict = None,
                            val_list=("0_0", "0_2"), test_list=("0_1", "0_3", "0_4", "0_5", "0_6", "0_7", "0_8", "0_9"), first_scored: int = 50,
                            reduce: bool = True):
        """main.py:279-415.  Two splits of the test infos -- 'Inner-val' (ids 0_0, 0_2) and 'Inner-test' (the other eight) --
        evaluated clip by clip (batch 1, all frames of the clip as the model's batch, main.py:361-365): per view the BCE-sum loss,
        pixel accuracy / Dice / precision / specificity / recall over ALL frames of the split and the per-part Dice
        (main.py:385-407).  net_root None (the call at the end of every training epoch, main.py:274): the current weights, returns
        the validation Dice averaged over views (main.py:409-410).  With net_root: every checkpoint net_%05d.pth found there is
        loaded and scored, and the best validation epoch from `first_scored` on is reported (main.py:412-415: epochs 50+).
        `infos`: the reference loads ./infos/test_infos.npy (NIfTI paths, not shipped); default = synthetic volumes with the same ids.
        reduce: sum the overlap counters over ranks (every rank must then make this call); False for a call made by one rank alone."""
        from .data import ContourAccumulator, SegPAHDataset, synthetic_infos, part_overlap_counts
        clip = 40 if raw_data else int(self.config["train"].get("clip_length", 40))                       # main.py:307-311
        if infos is None:
            infos = synthetic_infos(self.view_num, 10, clip, device="cpu", seed=91)
        splits = {"Inner-val": [i for i in val_list if i in infos], "Inner-test": [i for i in test_list if i in infos]}
        sets = {name: {v: SegPAHDataset(infos, is_train=False, data_list=ids, view_num=[v], single_frame=False, clip_length=clip + 1,
                                        seg_parts=True, device=self.device) for v in self.view_num} for name, ids in splits.items()}

        def score(tag):
            self.model.eval()
            report = {}
            for name, per_view in sets.items():
                counts = {v: torch.zeros(5, 4, dtype=torch.int64, device=self.device) for v in self.test_view}
                loss4view = {v: 0.0 for v in self.test_view}
                contour = {v: ContourAccumulator(5, self.device) for v in self.test_view} if self.contour_metrics else None
                for i in range(len(per_view[self.view_num[0]])):
                    imgs, masks = {}, {}
                    for v in self.view_num:
                        img, mask, _ = per_view[v][i]                          # [1,112,112,T], [5,112,112,T]
                        imgs[v] = img.permute(3, 0, 1, 2).contiguous()         # main.py:361-365: frames become the batch
                        masks[v] = mask.permute(3, 0, 1, 2).contiguous()
                    # every view draws its own clip window (loader.py:429-458), and one that runs past the end of its volume comes
                    # back short: the views keep their common leading frames (the model stacks the views frame by frame)
                    frames = min(t.shape[0] for t in imgs.values())
                    imgs = {v: t[:frames] for v, t in imgs.items()}
                    masks = {v: t[:frames] for v, t in masks.items()}
                    out = self._forward(imgs)
                    pred = self._prediction(out, is_fuse)
                    for v in self.test_view:
                        counts[v] += part_overlap_counts(pred[v], masks[v])
                        loss4view[v] += float(ops.bce_with_logits_sum(pred[v], masks[v]))
                        if contour is not None:
                            contour[v] += (pred[v], masks[v])
                res = {}
                contour_report = ContourAccumulator.reports(contour, reduce=reduce) if contour is not None else None
                for v in self.test_view:
                    # reduce=False: this rank scored every clip itself (the per-epoch call from train(), rank 0 only): no collective
                    per_part = all_reduce_counts(counts[v]) if reduce else counts[v]
                    res[v] = {"metrics": ops.overlap_metrics_from_counts(per_part.sum(dim=0)), "loss": loss4view[v],
                              "part_dice": [ops.overlap_metrics_from_counts(per_part[c])[1] for c in range(5)]}
                    if self.print_val:
                        m = res[v]["metrics"]
                        print(f"------Validation Result . {name} for view{v} {tag}------ Loss : {loss4view[v]:.4f} Pixel Acc : {m[0]:.4f} "
                              f"Dice : {m[1]:.4f} Precision : {m[2]:.4f} Specificity : {m[3]:.4f} Recall : {m[4]:.4f}; part dice "
                              + " ".join(f"{d:.4f}" for d in res[v]["part_dice"]))
                    if contour_report is not None:
                        res[v]["contour"] = contour_report[v]
                        if self.print_val:
                            print(f"------Validation Result . {name} for view{v} {tag}------ " + _contour_line(contour_report[v]))
                report[name] = res
            val = report["Inner-val"]
            report["val_dice"] = sum(val[v]["metrics"][1] for v in self.test_view) / max(len(self.test_view), 1)
            return report

        if net_root is None:
            self.validation_report = score("")
            return self.validation_report["val_dice"]
        dices = []
        for epoch in range(100):                                                # main.py:317
            path = os.path.join(net_root, "net_%05d.pth" % epoch)
            if not os.path.exists(path):
                break
            self.model.load_state_dict(torch.load(path, map_location=self.device)["network"], strict=True)
            dices.append(score(f"(epoch {epoch})")["val_dice"])
        scored = dices[first_scored:] if len(dices) > first_scored else dices
        off = first_scored if len(dices) > first_scored else 0
        best = max(range(len(scored)), key=lambda k: scored[k]) + off if scored else None
        if self.print_val and best is not None:
            print(f"best val epoch:{best},best val dice:{dices[best]}")
        return best, dices

    def _calculate_overlap_metrics(self, gt, logits, eps: float = 1e-5):
        """main.py:800-815 on pred = (sigmoid(logits) > 0.5); counters reduced over ranks."""
        counts = all_reduce_counts(ops.overlap_counts(logits, gt))
        return ops.overlap_metrics_from_counts(counts, eps)

    def save(self, epoch: int):
        """main.py:857-872: {'network': state_dict} -> save_dir/net_%05d.pth + latest.ckpt; with config['train']['save_optimizer']
        also {'epoch', 'optimizer': state_dict} -> opt_%05d.pth (the lines main.py:869-870 carries commented out; load() reads it)."""
        if not self.print_val:
            return
        d = self.config["train"]["save_dir"]
        os.makedirs(d, exist_ok=True)
        torch.save({"network": self.model.state_dict()}, os.path.join(d, "net_%05d.pth" % epoch))
        if self.save_optimizer:
            torch.save({"epoch": epoch, "optimizer": self.optimizer.state_dict()}, os.path.join(d, "opt_%05d.pth" % epoch))
        with open(os.path.join(d, "latest.ckpt"), "w") as f:
            f.write("%05d\n" % epoch)                              # main.py:869: `echo 00005 > latest.ckpt` (zero-padded, newline)

    def load(self):
        """main.py:823-855: resume from config['train']['save_dir'].  The latest epoch is the last line of latest.ckpt, else the
        highest net_*.pth; net_%05d.pth is loaded with strict=True, opt_%05d.pth into the optimizer when it exists (a checkpoint
        saved without config['train']['save_optimizer'] has none: one warning, the optimizer starts fresh).  train() then continues
        at the epoch after it, with the learning rate an uninterrupted run would have there: the scheduler takes the same
        `latest_epoch` steps from the base rate, so the recursion of CosineAnnealingLR yields the same bits.  Nothing found: one
        warning, `latest_epoch` stays 0."""
        d = self.config["train"]["save_dir"]
        latest = None
        if os.path.isfile(os.path.join(d, "latest.ckpt")):
            with open(os.path.join(d, "latest.ckpt")) as f:
                lines = f.read().split()
            latest = int(lines[-1]) if lines else None
        if latest is None:
            found = [int(os.path.basename(q)[4:-4]) for q in glob.glob(os.path.join(d, "net_*.pth")) if os.path.basename(q)[4:-4].isdigit()]
            latest = max(found) if found else None
        if latest is None:
            if self.print_val:
                print(f"Warning: no trained model found in {d}. An initialized model will be used.")
            self.latest_epoch = 0
            return
        net_path, opt_path = os.path.join(d, "net_%05d.pth" % latest), os.path.join(d, "opt_%05d.pth" % latest)
        if self.print_val:
            print(f"Loading model from {net_path}...")
        self.model.load_state_dict(torch.load(net_path, map_location=self.device)["network"], strict=True)
        if os.path.isfile(opt_path):
            self.optimizer.load_state_dict(torch.load(opt_path, map_location=self.device)["optimizer"])
        elif self.print_val:
            print(f"Warning: {opt_path} not found (saved without config['train']['save_optimizer']); the optimizer starts fresh.")
        ops.refresh_weights()                                      # load_state_dict copies in place: no stale weight image survives
        self.latest_epoch = latest + 1
        # the saved param_groups carry the rate of the moment of saving; the scheduler built in __init__ stands at step 0
        for group, base in zip(self.optimizer.param_groups, self.scheduler.base_lrs):
            group["lr"] = base
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)           # "lr_scheduler.step() before optimizer.step()": intended here
            for _ in range(self.latest_epoch):
                self.scheduler.step()
