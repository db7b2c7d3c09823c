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
"""
from __future__ import annotations

from typing import Dict, List

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


class _Fused(torch.optim.Optimizer):
    """What the fused optimizers share: the checks on a parameter and its gradient, one pointer table and one launch per
    (param group, class of parameters that take the same scalars), the version bump and the weight-image refresh.
    A subclass says, per parameter, which class it falls into and which state tensors go into the table (`_classify`),
    and launches its kernel over a class's table (`_launch`)."""
    _NAME = ""
    _SPARSE = ""

    def _classify(self, group: dict, p: torch.Tensor):
        """-> (class key, pointer for table column 2, pointer for column 3); creates / advances the parameter's state."""
        raise NotImplementedError

    def _launch(self, group: dict, key, table: torch.Tensor) -> None:
        raise NotImplementedError

    def _table_key(self, gi: int, key, n_classes: int) -> tuple:
        return (gi, key)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
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
                dev = p.device
                updated.append(p)
            for key, entries in classes.items():
                table = self._tables.setdefault(self._table_key(gi, key, len(classes)), _Table()).get(entries, dev)
                self._launch(group, key, table)
            if updated:
                # the kernel writes through raw pointers: tell autograd (and every cache keyed on `_version`: the
                # tap-major / transposed / pre-split weight layouts and the measured maxima in ops.py) that these changed
                torch.autograd.graph.increment_version(updated)
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
        check(lib.glf_adam_step(_p(table), table.shape[0], float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                float(group["weight_decay"]), t, _stream()), "adam_step")


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

    def _classify(self, group, p):
        """Class = "gets its first momentum buffer in this step" (the kernel writes it and never reads it) or not."""
        if group["momentum"] == 0:
            return False, 0, 0
        st = self.state[p]
        buf = st.get("momentum_buffer")
        first = buf is None
        if first:
            buf = torch.empty_like(p, memory_format=torch.contiguous_format)
        elif not buf.is_cuda or buf.dtype != torch.float32 or buf.numel() != p.numel():
            raise RuntimeError("glfusion_amd.optim.SGD: a momentum buffer must be a CUDA(HIP) float32 tensor of its parameter's size")
        elif not buf.is_contiguous():
            buf = buf.contiguous()
        st["momentum_buffer"] = buf
        return first, buf.data_ptr(), 0

    def _launch(self, group, first, table):
        if group.get("maximize"):
            raise NotImplementedError("glfusion_amd.optim.SGD: maximize is not used by the reference (main.py:159) and not built")
        check(lib.glf_sgd_step(_p(table), table.shape[0], float(group["lr"]), float(group["momentum"]), float(group["dampening"]),
                               float(group["weight_decay"]), int(bool(group["nesterov"])), int(first), _stream()), "sgd_step")
