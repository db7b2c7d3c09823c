"""Optimizer of the reference's training loop (GLfusion/main.py:158-169) on the HIP engine.

`Adam` has torch.optim.Adam's constructor, param_groups and state layout ('step', 'exp_avg', 'exp_avg_sq' per
parameter -- optimizer checkpoints are interchangeable with torch.optim.Adam's), so
`torch.optim.lr_scheduler.CosineAnnealingLR` (main.py:168) drives it unchanged; `step()` updates every parameter
that has a gradient with ONE kernel launch per (param group, step count) (glf_adam_step) instead of ~1 500 small
ATen kernels.  Parameters without a gradient are skipped and get no state, exactly as in torch (the dead
`network.*` template and `align_channel` never receive one on this path).

`SGD` is the other branch of main.py:158-161, built the same way: torch.optim.SGD's constructor, param_groups keys and
state ('momentum_buffer' per parameter, only with momentum != 0), one glf_sgd_step launch per (param group, "has a
momentum buffer" / "gets its first one").

Global-norm gradient clipping with a non-finite guard is opt-in on both (`set_grad_clip`) and stays on the device: one extra
read of the gradients (glf_grad_sumsq + glf_grad_clip_coef), the clip as one multiply inside the update kernels
(glf_adam_step_clipped / glf_sgd_step_clipped), the coefficient and the "skip this step" decision never seen by the host.
`grad_norm` and `clip_grad_norm_` are the same two norm launches as free functions for callers with their own loop.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch

from ._lib import check, lib
from .ops import _p, _stream, refresh_weights

CHUNK = 1 << 16          # elements per table row (one workgroup pass)


def _chunk_rows(entries: List[tuple]) -> np.ndarray:
    """(p_ptr, g_ptr, m_ptr, v_ptr, n) per parameter -> int64 table with one row per CHUNK elements."""
    a = np.asarray(entries, dtype=np.int64).reshape(-1, 5)
    n = a[:, 4]
    k = (n + CHUNK - 1) // CHUNK
    idx = np.repeat(np.arange(len(a)), k)
    first = np.cumsum(k) - k
    off = (np.arange(int(k.sum())) - np.repeat(first, k)) * CHUNK
    rows = a[idx].copy()
    rows[:, 0:4] += (off * 4)[:, None]
    rows[:, 4] = np.minimum(CHUNK, n[idx] - off)
    return rows


class _Table:
    """Device copy of a pointer table, re-uploaded only when a pointer changed (gradients that live in the
    all-reduce buckets never move; freshly allocated ones usually come back at the same addresses).  Uploads go
    through two alternating pinned host buffers so that step() never synchronises the host with the GPU."""

    def __init__(self):
        self.key = None
        self.dev = None
        self.host = [None, None]
        self.events = [None, None]
        self.turn = 0

    def get(self, entries: List[tuple], device) -> torch.Tensor:
        key = tuple(entries)
        if key == self.key:
            return self.dev
        rows = _chunk_rows(entries)
        i = self.turn
        self.turn ^= 1
        if self.host[i] is None or self.host[i].shape[0] < rows.shape[0]:
            self.host[i] = torch.empty(max(rows.shape[0], 64), 5, dtype=torch.int64).pin_memory()
            self.events[i] = None
        if self.events[i] is not None:
            self.events[i].synchronize()                    # the copy issued two uploads ago; long finished
        self.host[i][:rows.shape[0]].copy_(torch.from_numpy(rows))
        if self.dev is None or self.dev.shape[0] != rows.shape[0] or self.dev.device != device:
            self.dev = torch.empty(rows.shape[0], 5, dtype=torch.int64, device=device)
        self.dev.copy_(self.host[i][:rows.shape[0]], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[i] = ev
        self.key = key
        return self.dev


def _check_max_norm(max_norm) -> float:
    max_norm = float(max_norm)
    if math.isnan(max_norm) or max_norm < 0.0:
        raise ValueError(f"max_norm must be a non-negative number (float('inf') keeps only the non-finite guard), got {max_norm}")
    return max_norm


class _Norm:
    """The device side of one global gradient norm: the per-row partial sums, the record { norm, coef, ok, 0 } and the
    counter of non-finite norms.  `run` issues the two launches over one table; nothing is read back."""

    def __init__(self):
        self.partials = None
        self.record = None
        self.skipped = None

    def run(self, table: torch.Tensor, max_norm: float) -> torch.Tensor:
        n = table.shape[0]
        if self.record is None or self.record.device != table.device:
            self.partials = None
            self.record = torch.zeros(4, dtype=torch.float32, device=table.device)
            self.skipped = torch.zeros((), dtype=torch.int64, device=table.device)
        if self.partials is None or self.partials.shape[0] < n:
            self.partials = torch.empty(max(n, 64), dtype=torch.float64, device=table.device)
        check(lib.glf_grad_sumsq(_p(table), n, _p(self.partials), _stream()), "grad_sumsq")
        check(lib.glf_grad_clip_coef(_p(self.partials), n, max_norm, _p(self.record), _p(self.skipped), _stream()), "grad_clip_coef")
        return self.record


# a new momentum buffer under clipping: glf_sgd_step_clipped's "not written yet" mark (include/glfusion.h)
_UNBORN = 0x7fc0dead


class _Fused(torch.optim.Optimizer):
    """What the fused optimizers share: the checks on a parameter and its gradient, one pointer table and one launch per
    (param group, class of parameters that take the same scalars), the version bump and the weight-image refresh.
    A subclass says, per parameter, which class it falls into and which state tensors go into the table (`_classify`),
    and launches its kernel over a class's table (`_launch`).

    `set_grad_clip(max_norm)` makes every `step()` clip by the global L2 norm of all gradients (all param groups, all classes)
    and skip itself when that norm is not finite:
      * `p.grad` is left UNSCALED -- the coefficient min(1, max_norm / (norm + 1e-6)) is applied inside the update kernel.  This
        is the difference from `torch.nn.utils.clip_grad_norm_`, and the reason no gradient is rewritten.
      * `grad_norm`, `clip_coef` (device float32 scalars, views into the record) and `skipped_steps` (device int64 scalar)
        describe the last `step()` / count the skipped ones; reading them is the caller's synchronisation, `step()` has none.
      * a skipped step leaves parameters, moments and momentum buffers as they were.  The host cannot know of it: versions
        are bumped and the weight images refreshed all the same (harmless on unchanged weights), and Adam's host-side
        state['step'] still advances, so after a skipped step the bias correction is one step ahead.  A momentum buffer
        that SGD creates while clipping is on is filled with a NaN mark that the kernel reads as "first step"; it holds real
        values after the first step that is not skipped.
    It is deliberately not a param_groups / defaults key: state_dict() stays torch's."""
    _NAME = ""
    _SPARSE = ""
    _max_norm: Optional[float] = None
    _norm: Optional[_Norm] = None
    _record: Optional[torch.Tensor] = None       # the record of the step() in progress when it clips: _launch picks the clipped kernel

    def _classify(self, group: dict, p: torch.Tensor):
        """-> (class key, pointer for table column 2, pointer for column 3); creates / advances the parameter's state."""
        raise NotImplementedError

    def _launch(self, group: dict, key, table: torch.Tensor) -> None:
        """One update launch; with `self._record` set (a clipped step) the clipped kernel over that record."""
        raise NotImplementedError

    def _table_key(self, gi: int, key, n_classes: int) -> tuple:
        return (gi, key)

    def set_grad_clip(self, max_norm: Optional[float]) -> None:
        """Clip every following step() by the global gradient norm `max_norm` and skip steps whose norm is not finite;
        float('inf') keeps only the guard, None switches both off again."""
        if max_norm is None:
            self._settle_unborn()
            self._max_norm = None
            return
        self._max_norm = _check_max_norm(max_norm)
        if self._norm is None:
            self._norm = _Norm()

    def _settle_unborn(self) -> None:
        """Leaving clipped mode: nothing to settle unless a subclass creates marked state."""

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """Global gradient norm of the last clipped step(): a device float32 scalar (None before the first one)."""
        return None if self._norm is None or self._norm.record is None else self._norm.record[0]

    @property
    def clip_coef(self) -> Optional[torch.Tensor]:
        """The coefficient the last clipped step() multiplied its gradients by (0 for a skipped step): a device float32 scalar."""
        return None if self._norm is None or self._norm.record is None else self._norm.record[1]

    @property
    def skipped_steps(self) -> Optional[torch.Tensor]:
        """Number of clipped step() calls skipped for a non-finite norm: a device int64 scalar (None before the first one)."""
        return None if self._norm is None else self._norm.skipped

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        any_dev = None
        for gi, group in enumerate(self.param_groups):
            classes: Dict[object, List[tuple]] = {}
            dev = None
            updated = []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError(self._SPARSE)
                if not p.is_cuda or p.dtype != torch.float32 or g.dtype != torch.float32:
                    raise RuntimeError(f"glfusion_amd.optim.{self._NAME}: parameters and gradients must be CUDA(HIP) float32 tensors "
                                       "(the engine has no CPU fallback)")
                if not p.is_contiguous():
                    raise RuntimeError(f"glfusion_amd.optim.{self._NAME}: non-contiguous parameter")
                if not g.is_contiguous():
                    g = g.contiguous()
                    p.grad = g
                key, m_ptr, v_ptr = self._classify(group, p)
                classes.setdefault(key, []).append((p.data_ptr(), g.data_ptr(), m_ptr, v_ptr, p.numel()))
                dev = any_dev = p.device
                updated.append(p)
            tables = [(key, self._tables.setdefault(self._table_key(gi, key, len(classes)), _Table()).get(entries, dev), entries)
                      for key, entries in classes.items()]
            work.append((group, tables, updated))
        n_tables = sum(len(tables) for _, tables, _ in work)
        if self._max_norm is not None and n_tables:
            # ONE norm over every gradient of this step: the update's own table in the usual single-class case, else a combined one
            if n_tables == 1:
                table = next(t for _, tables, _ in work for _, t, _ in tables)
            else:
                entries = [e for _, tables, _ in work for _, _, es in tables for e in es]
                table = self._tables.setdefault(("norm",), _Table()).get(entries, any_dev)
            self._record = self._norm.run(table, self._max_norm)
        try:
            for group, tables, updated in work:
                for key, table, _ in tables:
                    self._launch(group, key, table)
                if updated:
                    # the kernel writes through raw pointers: tell autograd (and every cache keyed on `_version`: the
                    # tap-major / transposed / pre-split weight layouts and the measured maxima in ops.py) that these changed
                    torch.autograd.graph.increment_version(updated)
        finally:
            self._record = None
        # ... and rebuild every registered weight-derived image in four launches (instead of ~5 launches per conv when the
        # next forward finds its caches stale)
        refresh_weights()
        return loss


class Adam(_Fused):
    _NAME = "Adam"
    _SPARSE = "Adam does not support sparse gradients, please consider SparseAdam instead"

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid Adam hyper-parameter")           # torch.optim.Adam raises ValueError too
        if amsgrad:
            raise NotImplementedError("glfusion_amd.optim.Adam: amsgrad is not used by the reference (main.py:162) and not built")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False))
        self._tables: Dict[tuple, _Table] = {}

    def _table_key(self, gi, t, n_classes):
        return (gi, n_classes > 1 and t)               # t moves every step: the usual single class keeps ONE table

    def _classify(self, group, p):
        """Class = the step count t (torch keeps one per parameter; the bias corrections depend on it)."""
        st = self.state[p]
        if len(st) == 0:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        t = int(st["step"]) + 1
        st["step"] = st["step"].new_tensor(float(t)) if isinstance(st["step"], torch.Tensor) else t
        return t, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()

    def _launch(self, group, t, table):
        b1, b2 = group["betas"]
        args = (_p(table), table.shape[0], float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), t)
        if self._record is None:
            check(lib.glf_adam_step(*args, _stream()), "adam_step")
        else:
            check(lib.glf_adam_step_clipped(*args, _p(self._record), _stream()), "adam_step_clipped")


class SGD(_Fused):
    _NAME = "SGD"
    _SPARSE = "glfusion_amd.optim.SGD: sparse gradients are not built"

    def __init__(self, params, lr: float, momentum: float = 0, dampening: float = 0, weight_decay: float = 0,
                 nesterov: bool = False):
        # torch.optim.SGD's own checks (the same ValueErrors) and its own param_groups keys, whatever this torch version carries
        # beyond the five that are built: a throw-away instance over one CPU scalar
        twin = torch.optim.SGD([torch.zeros(1)], lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                               nesterov=nesterov)
        super().__init__(params, dict(twin.defaults))
        self._tables: Dict[tuple, _Table] = {}
        self._unborn: List[tuple] = []                   # (parameter, momentum buffer created while clipping was on)

    def _classify(self, group, p):
        """Class = "gets its first momentum buffer in this step" (the kernel writes it and never reads it) or not."""
        if group["momentum"] == 0:
            return False, 0, 0
        st = self.state[p]
        buf = st.get("momentum_buffer")
        first = buf is None
        if first:
            buf = torch.empty_like(p, memory_format=torch.contiguous_format)
            if self._max_norm is not None:
                # this step may be skipped on the device: the mark keeps the buffer a "first" one for the kernel until it is written
                buf.view(torch.int32).fill_(_UNBORN)
                self._unborn.append((p, buf))
        elif not buf.is_cuda or buf.dtype != torch.float32 or buf.numel() != p.numel():
            raise RuntimeError("glfusion_amd.optim.SGD: a momentum buffer must be a CUDA(HIP) float32 tensor of its parameter's size")
        elif not buf.is_contiguous():
            buf = buf.contiguous()
        st["momentum_buffer"] = buf
        return first, buf.data_ptr(), 0

    def _launch(self, group, first, table):
        if group.get("maximize"):
            raise NotImplementedError("glfusion_amd.optim.SGD: maximize is not used by the reference (main.py:159) and not built")
        args = (_p(table), table.shape[0], float(group["lr"]), float(group["momentum"]), float(group["dampening"]),
                float(group["weight_decay"]), int(bool(group["nesterov"])), int(first))
        if self._record is None:
            check(lib.glf_sgd_step(*args, _stream()), "sgd_step")
        else:
            check(lib.glf_sgd_step_clipped(*args, _p(self._record), _stream()), "sgd_step_clipped")

    def _settle_unborn(self) -> None:
        """Clipping goes off: a buffer created under it whose every step was skipped still holds the mark, which only the
        clipped kernel understands.  Such a buffer leaves the state again (the next step is then a first step, as in torch).
        This reads the device once; it is not on the step() path."""
        for p, buf in self._unborn:
            st = self.state.get(p)
            if st is not None and st.get("momentum_buffer") is buf and int(buf.view(torch.int32).view(-1)[0]) == _UNBORN:
                del st["momentum_buffer"]
        self._unborn = []


def _grad_table(parameters: Iterable[torch.Tensor], what: str):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    entries, dev = [], None
    for p in parameters:
        g = p.grad
        if g is None:
            continue
        if not g.is_cuda or g.dtype != torch.float32 or g.is_sparse:
            raise RuntimeError(f"glfusion_amd.optim.{what}: gradients must be dense CUDA(HIP) float32 tensors (the engine has no CPU fallback)")
        if not g.is_contiguous():
            g = g.contiguous()
            p.grad = g
        entries.append((0, g.data_ptr(), 0, 0, g.numel()))
        dev = g.device
    if not entries:
        raise RuntimeError(f"glfusion_amd.optim.{what}: no parameter has a gradient")
    return _Table().get(entries, dev)


def grad_norm(parameters: Iterable[torch.Tensor]) -> torch.Tensor:
    """Global L2 norm of the parameters' gradients as a device float32 scalar: one table upload, two launches (glf_grad_sumsq,
    glf_grad_clip_coef), double accumulation in a fixed order, no host synchronisation."""
    return _Norm().run(_grad_table(parameters, "grad_norm"), math.inf)[0]


def clip_grad_norm_(parameters: Iterable[torch.Tensor], max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type 2) without its ~1 500 launches and without a host
    synchronisation: the norm as in `grad_norm`, then ONE launch that scales every .grad in place by
    min(1, max_norm / (norm + 1e-6)) (glf_grad_scale).  Returns the norm as a device float32 scalar.  With a non-finite norm
    the gradients are left unchanged (torch would write NaNs into all of them)."""
    max_norm = _check_max_norm(max_norm)
    table = _grad_table(parameters, "clip_grad_norm_")
    record = _Norm().run(table, max_norm)
    check(lib.glf_grad_scale(_p(table), table.shape[0], _p(record), _stream()), "grad_scale")
    return record[0]
