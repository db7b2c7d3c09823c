"""torch.autograd.Function wrappers over the C ABI (include/glfusion.h).

Every function here launches hand-written gfx950 kernels from libglfusion_hip.so on
PyTorch's current HIP stream.  PyTorch is used for device memory (torch.empty / zeros),
views and the autograd graph only.  Inputs that are not CUDA float32 tensors raise: there
is no CPU or eager fallback on the product path.

Internal layout: activations are channels-last, carried as contiguous [N, H, W, C]
tensors (== the row-major matrix [N*H*W, C] the kernels see).
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import List, Optional, Sequence, Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import conv_plan
from ._lib import GemmEpilogue, GemmParams, SEG_MAX, TN_OIHW_MAX_TAPS, WeightJob, WJ_AMAX, WJ_COPY, WJ_PACK, WJ_PASSES, WJ_PASS_OF, WJ_TAP_MAJOR, WJ_TAP_MAJOR_T, WJ_TRANSPOSE, WJ_ZERO, check, lib
from .conv_plan import CENTRE_TAP, RECT_THRESHOLD, rect_fraction, tap_mask          # re-exported: the same objects, the rules live in conv_plan


# ----------------------------------------------------------------------------------------
# small helpers
# ----------------------------------------------------------------------------------------
BF = torch.bfloat16
DT_F32, DT_BF16 = 0, 1                  # GLF_DT_* of include/glfusion.h


def _is16(t) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype == BF


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t: torch.Tensor, name: str = "tensor", dtype: Optional[torch.dtype] = torch.float32) -> torch.Tensor:
    """t must be a CUDA tensor of `dtype`; dtype=None: of either storage dtype (the streaming nodes serve fp32 and bf16 alike)."""
    if dtype is None:
        dtype = BF if _is16(t) else torch.float32
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
        kind = "bfloat16 tensor in 16-bit storage mode" if dtype == BF else "float32 tensor"
        raise RuntimeError(f"glfusion_amd: {name} must be a CUDA(HIP) {kind} (got "
                           f"{getattr(t, 'device', None)}, {getattr(t, 'dtype', None)}). The engine has no CPU fallback.")
    return t


def _contig(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _ws(rows: int, c: int, dev) -> torch.Tensor:
    return torch.empty(int(lib.glf_bn_workspace(rows, c)), dtype=torch.float64, device=dev)


def zeros(*shape, dtype=torch.float32, device=None) -> torch.Tensor:
    """Zero-filled device tensor through the library (glf_zero on the current stream), for accumulation targets."""
    t = torch.empty(*shape, dtype=dtype, device=device)
    if t.numel():
        check(lib.glf_zero(_p(t), t.numel() * t.element_size(), _stream()), "zero")
    return t


def zero_(t: torch.Tensor) -> torch.Tensor:
    """In-place zero of a DENSE tensor (contiguous storage span) through the library."""
    if not t.is_contiguous():
        raise RuntimeError("glfusion_amd: zero_ needs a contiguous tensor")
    if t.numel():
        check(lib.glf_zero(_p(t), t.numel() * t.element_size(), _stream()), "zero")
    return t


def _dt(t: torch.Tensor) -> int:
    return DT_BF16 if t.dtype == BF else DT_F32


# The streaming ops between the contractions have one entry point per storage dtype: glf_<name> for fp32, glf_s16_<name> for bf16,
# with the same argument list -- except these, given here as (bf16 name, arguments) in terms of the fp32 call's arguments:
# the 16-bit row sums / broadcasts take the dtype of their fp32-or-bf16 side, and glf_copy_frames moves 16-byte pieces counted in
# floats (a bf16 extent is half as long).
_S16_FORM = {
    "avgpool_fwd": lambda x, y, n, p, c: ("s16_sum_rows", (x, c, y, _dt(y), 1.0 / p, n, p, c)),
    "sum_rows_fwd": lambda x, ld, y, scale, n, p, c: ("s16_sum_rows", (x, ld, y, _dt(y), scale, n, p, c)),
    "bcast_rows_scaled": lambda x, y, ld, scale, n, p, c: ("s16_bcast_rows", (x, _dt(x), y, ld, scale, n, p, c)),
    "copy_frames": lambda src, sfs, dst, dfs, n, inner: ("copy_frames", (src, sfs // 2, dst, dfs // 2, n, inner // 2)),
}


def _launch(name: str, ref: torch.Tensor, *args) -> None:
    """Launch streaming op `name` (named after its fp32 entry point glf_<name>) for the storage dtype of `ref` on the current
    stream.  Tensors are passed as tensors.  The ONE place where a node's dtype picks its kernel."""
    if _is16(ref):
        name, args = _S16_FORM[name](*args) if name in _S16_FORM else ("s16_" + name, args)
    check(getattr(lib, "glf_" + name)(*[_p(a) if isinstance(a, torch.Tensor) else a for a in args], _stream()), name)


def to_nhwc(x: torch.Tensor) -> torch.Tensor:
    """NCHW-shaped tensor (any strides) -> contiguous [N,H,W,C]; free for channels_last / C == 1."""
    _chk(x, "input")
    if x.dim() != 4:
        raise RuntimeError(f"expected a 4-D NCHW tensor, got shape {tuple(x.shape)}")
    n, c, h, w = x.shape
    if c == 1:
        return _contig(x).reshape(n, h, w, 1)
    xp = x.permute(0, 2, 3, 1)
    return xp if xp.is_contiguous() else xp.contiguous()


def from_nhwc(y: torch.Tensor) -> torch.Tensor:
    """[N,H,W,C] -> NCHW-shaped view with channels_last strides (zero-copy)."""
    return y.permute(0, 3, 1, 2)


# ----------------------------------------------------------------------------------------
# contraction front-end
# ----------------------------------------------------------------------------------------
# contraction precision of the calls this module issues (index into PRECISIONS); passed PER CALL through
# glf_gemm_params.precision, so nothing process-wide is touched in the library
_PREC = [0]
_S16 = [False]             # 16-bit storage mode ("bf16" precision): see glfusion_amd.ops16


def s16() -> bool:
    return _S16[0]


def act_dtype() -> torch.dtype:
    """dtype of the activations the engine keeps in HBM under the current precision."""
    return torch.bfloat16 if _S16[0] else torch.float32


# bench.py sets this to a list to time every contraction launch with HIP events on the launch stream
PROFILER = None
KERNEL_NAMES = {("nt", False): "gemm_rows_kernel<0,false>", ("nt", True): "gemm_rows_kernel<0,true>",
                ("nn", False): "gemm_rows_kernel<1,false>", ("nn", True): "gemm_rows_kernel<1,true>",
                ("tn", False): "gemm_tn_kernel<false>", ("tn", True): "gemm_tn_kernel<true>"}


def gemm(mode: str, A: torch.Tensor, B: torch.Tensor, Cm: torch.Tensor, *, M: int, N: int, K: int,
         lda: int, ldb: int, ldc: int, bias: Optional[torch.Tensor] = None, taps: int = 1, mask: int = 1,
         tap_stride_b: int = 0, gather: int = 0, geo: Optional[Tuple[int, ...]] = None, batch: int = 1,
         bsa: int = 0, bsb: int = 0, bsc: int = 0, alpha: float = 1.0, accumulate: bool = False,
         split: int = 1, rect: bool = False, amax_a: Optional[torch.Tensor] = None,
         amax_b: Optional[torch.Tensor] = None, amax_c: Optional[torch.Tensor] = None,
         colstats: Optional[torch.Tensor] = None, a_packed: bool = False, b_packed: bool = False,
         colmax: Optional[torch.Tensor] = None, epilogue=None, oihw: bool = False, foreign=None, seg=None, seg_cols=None) -> bool:
    """mode in {'nt','nn','tn'}; geo = (n_img, hs, ws, hd, wd, kh, kw, stride, pad, dil).
    epilogue ('nt' only): (residual or None, its row stride, relu) -- the call goes to glf_gemm_nt_epilogue, which stores
    act(alpha * acc + bias[n] + residual[m][n]) once (bias is then required: the folded BatchNorm shift).
    amax_a / amax_b: device scalars bounding max|A| / max|B| (f16x3 precision only; None = measured by the library);
    amax_c: a slot from amax_slot() that receives max|C written| (ignored by rect / split > 1 / non-f16x3 calls -- pass
    it only to calls that store C directly).
    a_packed / b_packed: A / B is the packed pre-split image packed_of() made with the same amax_a / amax_b.
    oihw ('tn' only, see tn_oihw_ok): Cm is the parameter-shaped [M][N][taps] gradient -- the second stage of the reduction
    stores every tap of an element side by side, zeros for the taps outside `mask` (which may then be empty: nothing is
    contracted); foreign = (tap, src, row stride): that tap's [M][N] values are copied from src.
    seg ('nt' only, glf_gemm_params.nseg): (kx, [(oy, ox, acol), ...], dense FLOPs, executed FLOPs) -- the segmented region
    mode over the geo = (n_img, h, w, h, w, 1, 1, 1, 0, 1) map; the two FLOP counts are what the profiler record carries.  A
    launch the library refuses as unsupported returns False (nothing ran: the caller takes its other route); every other
    call returns True.
    seg_cols (with seg, glf_gemm_nt_seg_cols): [(first column, columns, B offset), ...], one per segment -- the segment adds to
    that group of output columns only and reads its slice of B at that offset from the start of a column's row."""
    p = GemmParams()
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc = M, N, K, lda, ldb, ldc
    p.taps, p.tap_mask, p.tap_stride_b, p.gather = taps, mask, tap_stride_b, gather
    if geo is not None:
        (p.n_img, p.hs, p.ws, p.hd, p.wd, p.kh, p.kw, p.stride, p.pad, p.dil) = geo
    else:
        (p.n_img, p.hs, p.ws, p.hd, p.wd, p.kh, p.kw, p.stride, p.pad, p.dil) = (1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    p.batch, p.batch_stride_a, p.batch_stride_b, p.batch_stride_c = batch, bsa, bsb, bsc
    p.alpha, p.accumulate, p.split, p.rect = alpha, int(accumulate), split, int(rect)
    p.amax_a, p.amax_b, p.amax_c = _p(amax_a), _p(amax_b), _p(amax_c)
    p.colstats = _p(colstats)                  # zero-filled float64 [2, N]: column sums of C and C^2 (f16x3 NT only)
    p.colmax = _p(colmax)                      # zero-filled float32 [N]: column maxima of |C| (with colstats)
    p.precision = _PREC[0] + 1
    p.a_presplit, p.b_presplit = int(a_packed), int(b_packed)
    if oihw:
        if mode != "tn":
            raise ValueError("gemm: the parameter-layout store exists for mode 'tn' only")
        p.c_oihw = 1
        if foreign is not None:
            p.foreign_tap, p.foreign_src, p.foreign_ld = int(foreign[0]), _p(foreign[1]), int(foreign[2])
    if seg is not None:
        if mode != "nt":
            raise ValueError("gemm: segments exist for mode 'nt' only")
        seg_arr = (C.c_int32 * (3 * len(seg[1])))(*[v for t in seg[1] for v in t])
        p.nseg, p.seg_kx, p.seg = len(seg[1]), int(seg[0]), C.cast(seg_arr, C.c_void_p)
        if seg_cols is not None:
            if bias is not None or epilogue is not None or len(seg_cols) != len(seg[1]):
                raise ValueError("gemm: column groups take one (first column, columns, B offset) per segment, no bias, no epilogue")
            cols_arr = (C.c_int32 * (2 * len(seg_cols)))(*[v for t in seg_cols for v in t[:2]])
            boff_arr = (C.c_int64 * len(seg_cols))(*[t[2] for t in seg_cols])
    elif seg_cols is not None:
        raise ValueError("gemm: column groups belong to a segmented launch (seg=)")
    ws = None
    if mode == "tn" and (split > 1 or oihw) and mask:
        # two-stage reduction: the slices store partial sums, a second kernel adds them in a fixed order -- no atomics, no
        # zero-filled C, bitwise reproducible gradients
        nbytes = int(lib.glf_gemm_tn_workspace_bytes(C.byref(p)))
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=Cm.device)
        p.workspace, p.workspace_bytes = _p(ws), nbytes
    prof = PROFILER if mask else None          # (an empty mask contracts nothing: the store-only form of the TN second stage)
    if prof is not None:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev0.record()
    if mode == "nt" and epilogue is not None:
        e = GemmEpilogue()
        e.shift, e.residual, e.ld_res, e.relu = _p(bias), _p(epilogue[0]), int(epilogue[1]), int(bool(epilogue[2]))
        check(lib.glf_gemm_nt_epilogue(_p(A), _p(B), _p(Cm), C.byref(p), C.byref(e), _stream()), "gemm_nt_epilogue")
    elif epilogue is not None:
        raise ValueError("gemm: the fused epilogue exists for mode 'nt' only")
    elif mode == "nt":
        if seg_cols is not None:
            rc = lib.glf_gemm_nt_seg_cols(_p(A), _p(B), _p(Cm), C.byref(p), C.cast(cols_arr, C.c_void_p), C.cast(boff_arr, C.c_void_p), _stream())
        else:
            rc = lib.glf_gemm_nt(_p(A), _p(B), _p(bias), _p(Cm), C.byref(p), _stream())
        if seg is not None and rc == -2:          # GLF_ERR_UNSUPPORTED
            return False
        check(rc, "gemm_nt")
    elif mode == "nn":
        check(lib.glf_gemm_nn(_p(A), _p(B), _p(bias), _p(Cm), C.byref(p), _stream()), "gemm_nn")
    elif mode == "tn":
        check(lib.glf_gemm_tn(_p(A), _p(B), _p(Cm), C.byref(p), _stream()), "gemm_tn")
    else:
        raise ValueError(mode)
    if prof is not None:
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        # dense, reference-equivalent FLOPs of this launch (every tap, padding included), the FLOPs of the taps the
        # host-side mask keeps, and the ALGORITHMIC bytes: every operand element read once, every result written once
        kept_taps = bin(mask).count("1")
        dense = 2.0 * M * N * K * taps * batch
        src_rows = (geo[0] * geo[1] * geo[2]) if geo else None
        # per-tap rectangle / region launches contract only the in-range part of every kept tap: the EXECUTED work is the
        # kept taps' work times that fraction (ASPP rate 12: 0.51, rate 24: 0.18)
        in_range = rect_fraction(gather, geo[3], geo[4], geo[1], geo[2], geo[5], geo[6], geo[8], geo[9], mask) if (rect and geo and gather) else 1.0
        if mode == "tn":
            abytes = 4.0 * batch * (K * M + (src_rows if src_rows else K) * N + M * N * kept_taps)
        else:
            abytes = 4.0 * batch * ((src_rows if src_rows else M) * K + N * K * kept_taps + M * N * (2 if accumulate else 1))
        executed = dense * kept_taps / taps * in_range
        if seg is not None:
            dense, executed = float(seg[2]), float(seg[3])
            abytes = 4.0 * (M * lda + N * (K + len(seg[1]) * seg[0]) + M * N)
            if seg_cols is not None:           # a segment's slice exists for its own columns only
                abytes = 4.0 * (M * lda + N * K + seg[0] * sum(t[1] for t in seg_cols) + M * N)
        prof.append((KERNEL_NAMES[(mode, gather != 0)], dense, executed, ev0, ev1,
                     (M, N, K, taps, kept_taps, batch, split, geo[8] if geo else 0, geo[9] if geo else 0), abytes))
    return True


# ----------------------------------------------------------------------------------------
# weight-derived images: caches + the multi-tensor refresh (include/glfusion.h: glf_weights_refresh)
# ----------------------------------------------------------------------------------------
# Everything derived from a parameter -- its max magnitude (f16x3 / f16), the tap-major re-layouts of a k x k weight, the
# transposed copy of a 1x1 / linear weight, the stacked theta | phi | g operand, and the packed pre-split images of those --
# is cached against the parameter's version counter and rebuilt after an optimizer step.  One image at a time that is a
# launch per image (~1 000 per update for the 3-view model); every image therefore also registers itself as a JOB of a device
# table, and refresh_weights() recomputes all registered images in four launches.  An image keeps its buffer for the life of
# its parameter (a miss recomputes IN PLACE), so the table -- and a hipGraph that captured a refresh -- stay valid.
class _WImage:
    __slots__ = ("key", "owner", "kind", "src", "dst", "amax", "dims", "version", "extra", "__weakref__")


class _WeightRegistry:
    ARENA = 1 << 14

    def __init__(self, dev):
        self.dev = dev
        self.images = {}                   # key -> _WImage
        self.dirty = True
        self.arena = None                  # float32 [ARENA]: one slot per measured parameter
        self.free = []
        self.table = None                  # (device table, pass_first, pass_count, pass_wgs, n_jobs)

    def slot(self) -> torch.Tensor:
        if self.arena is None:
            self.arena = zeros(self.ARENA, device=self.dev)
            self.free = list(range(self.ARENA - 1, -1, -1))
        if not self.free:
            raise RuntimeError("glfusion_amd: weight amax arena exhausted (more than 16384 live parameters on one device)")
        i = self.free.pop()
        return self.arena[i:i + 1]

    def drop(self, key) -> None:
        try:
            im = self.images.pop(key, None)
        except (AttributeError, TypeError):      # interpreter shutdown: module globals are already gone
            return
        if im is not None:
            self.dirty = True
            if im.kind == 1 and self.arena is not None and im.amax is not None:        # 1 == WJ_AMAX (a literal: see drop at shutdown)
                self.free.append(int((im.amax.data_ptr() - self.arena.data_ptr()) // 4))

    def build(self, only=None):
        """Plan the job table of the registered images and copy it to the device.  only = None: all of them, installed as the
        registry's own table (rebuilt whenever an image is added or dropped; its refresh zero-fills the whole amax arena).
        only = a set of owner ids: a FROZEN table of those owners' images, returned to the caller together with strong
        references to every buffer it names -- what a captured hipGraph replays against (engine.StepGraph), valid however
        the registry changes afterwards; it zeroes exactly its own amax slots (GLF_WJ_ZERO jobs)."""
        ims = [im for im in self.images.values() if only is None or _image_belongs(im, only)]
        jobs = []                                  # (kind, src ptr, dst ptr, amax ptr, dims)
        for im in ims:
            jobs.append((im.kind, im.src.data_ptr(), im.dst.data_ptr() if im.dst is not None else 0,
                         im.amax.data_ptr() if im.amax is not None else 0, im.dims))
            if only is not None and im.kind == WJ_AMAX:
                jobs.append((WJ_ZERO, 0, im.amax.data_ptr(), 0, (1, 0, 0)))
        jobs.sort(key=lambda j: WJ_PASS_OF[j[0]])
        n = len(jobs)
        arr = (WeightJob * max(n, 1))()
        for j, (kind, src, dst, am, dims) in zip(arr, jobs):
            j.src, j.dst, j.amax, j.kind, j.pass_ = src, dst, am, kind, WJ_PASS_OF[kind]
            j.d0, j.d1, j.d2 = dims
        pf, pc, pw = (C.c_int * WJ_PASSES)(), (C.c_int * WJ_PASSES)(), (C.c_int64 * WJ_PASSES)()
        check(lib.glf_weights_plan(C.cast(arr, C.c_void_p), n, C.cast(pf, C.c_void_p), C.cast(pc, C.c_void_p), C.cast(pw, C.c_void_p)), "weights_plan")
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        table = (host.to(self.dev), pf, pc, pw, n)
        if only is not None:
            return table + ([(im.src, im.dst, im.amax) for im in ims], self.arena)
        self.table = table
        self.dirty = False
        return None

    def refresh(self, frozen=None) -> None:
        if frozen is not None:                     # a frozen table: no bookkeeping (its owner re-stamps nothing; eager callers
            tab, pf, pc, pw, n = frozen[:5]        # of the same parameters find their caches stale and rebuild in place)
            if n:
                check(lib.glf_weights_refresh(_p(tab), C.cast(pf, C.c_void_p), C.cast(pc, C.c_void_p), C.cast(pw, C.c_void_p),
                                              None, 0, _stream()), "weights_refresh")
            return
        if torch.cuda.is_current_stream_capturing() and self.dirty:
            raise RuntimeError("glfusion_amd: the weight-image table changed inside a graph capture (freeze a table first)")
        if self.dirty:
            self.build()
        tab, pf, pc, pw, n = self.table
        if n:
            check(lib.glf_weights_refresh(_p(tab), C.cast(pf, C.c_void_p), C.cast(pc, C.c_void_p), C.cast(pw, C.c_void_p),
                                          _p(self.arena), self.ARENA if self.arena is not None else 0, _stream()), "weights_refresh")
        for im in self.images.values():
            o = im.owner()
            if o is not None:
                im.version = _wversion(o, im)
                if im.kind == WJ_AMAX:
                    o._glf_amax = (o._version, o.data_ptr(), im.amax)


def _image_belongs(im, owner_ids) -> bool:
    """True when the image derives from one of the given parameters: directly, or through a stacked operand assembled from
    them (fusion._qkv_weights marks it with `_glf_sources`)."""
    o = im.owner()
    if o is None:
        return False
    if id(o) in owner_ids:
        return True
    srcs = getattr(o, "_glf_sources", None)
    return srcs is not None and any(r() is not None and id(r()) in owner_ids for r in srcs)


_wreg = {}


def _registry(dev) -> _WeightRegistry:
    r = _wreg.get(dev)
    if r is None:
        r = _wreg[dev] = _WeightRegistry(dev)
    return r


def _wversion(owner, im=None):
    """Version stamp of an image owner: the tensor's in-place counter, or -- for a dense operand ASSEMBLED from several
    parameters (fusion._qkv_weights sets `_glf_version_fn` on it) -- the combined stamp of its sources."""
    fn = getattr(owner, "_glf_version_fn", None)
    return fn() if fn is not None else owner._version


def _wimage(owner: torch.Tensor, tag: str, kind: int, src: torch.Tensor, dims, make_dst, amax: Optional[torch.Tensor] = None):
    """The cached image (owner, tag): (image, fresh) with fresh = False when the cached contents are current.  A stale or new
    image must be (re)computed by the caller into image.dst -- the buffer of a stale image is reused."""
    reg = _registry(owner.device)
    key = (id(owner), tag)
    im = reg.images.get(key)
    ver = _wversion(owner)
    if im is not None and im.owner() is owner and im.src.data_ptr() == src.data_ptr() and im.dims == tuple(dims) and \
            (im.amax is amax or kind == WJ_AMAX):
        if im.version == ver:
            return im, False
        im.version = ver
        return im, True
    if im is not None:
        reg.drop(key)
    im = _WImage()
    im.key, im.kind, im.src, im.dims, im.version, im.extra = key, kind, src, tuple(dims), ver, None
    im.owner = weakref.ref(owner, lambda _r, k=key, r=reg: r.drop(k))
    im.amax = reg.slot() if kind == WJ_AMAX else amax
    im.dst = make_dst() if make_dst is not None else None
    reg.images[key] = im
    reg.dirty = True
    return im, True


def refresh_weights(frozen=None) -> None:
    """Recompute every registered weight-derived image from the current parameter values (four launches per device on the
    current stream) and mark the caches current.  Call after an optimizer step wrote the parameters (glfusion_amd.optim.Adam
    does); anything not registered yet is still rebuilt lazily by its cache.  frozen: a table from freeze_weight_table() --
    only that table's images are recomputed (no cache bookkeeping): the form a captured step replays."""
    if frozen is not None:
        for dev, tab in frozen.items():
            _registry(dev).refresh(tab)
        return
    for reg in list(_wreg.values()):
        if reg.images:
            reg.refresh()


def reset_weight_images() -> None:
    """Forget every registered weight-derived image (they are rebuilt lazily by their caches): after a change of precision the
    images of the previous one would otherwise keep being refreshed with every update."""
    for reg in _wreg.values():
        for key in list(reg.images):
            reg.drop(key)


def freeze_weight_table(params) -> dict:
    """{device: frozen job table} of every image currently registered for the given parameters (run a step first so that
    they exist).  The tables hold their buffers alive; pass the dict to refresh_weights(frozen=...)."""
    ids = {id(p) for p in params}
    out = {}
    for dev, reg in _wreg.items():
        tab = reg.build(only=ids)
        if tab[4]:
            out[dev] = tab
    return out


def _is_weight(t: torch.Tensor) -> bool:
    return isinstance(t, torch.nn.Parameter) or hasattr(t, "_glf_version_fn")


def weight_amax(t: torch.Tensor) -> Optional[torch.Tensor]:
    """amax_of for a parameter (or a dense operand assembled from parameters): the scalar lives in the registry's arena."""
    if _PREC[0] < 2 or not t.is_contiguous():
        return None
    im, fresh = _wimage(t, "amax", WJ_AMAX, t, (t.numel(), 0, 0), None)
    if fresh:
        zero_(im.amax)
        check(lib.glf_amax(_p(t), 1, t.numel(), t.numel(), _p(im.amax), _stream()), "amax")
    return im.amax


def amax_of(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """Device scalar max|t| for the f16x3 contraction kernels (None under the other precisions, where it is not
    used).  Measured once per tensor and version and remembered on the tensor object; a permutation of the
    elements (weight re-layouts) has the same maximum, so callers pass the owning parameter.  Only call it on
    tensors whose contents are final (raw kernel writes do not bump torch's version counter)."""
    if t is None or _PREC[0] < 2:
        return None
    if _is_weight(t) and t.is_contiguous():
        return weight_amax(t)
    hit = getattr(t, "_glf_amax", None)
    if hit is not None and hit[0] == t._version and hit[1] == t.data_ptr():
        return hit[2]
    out = torch.empty(1, dtype=torch.float32, device=t.device)
    if t.is_contiguous():
        check(lib.glf_amax(_p(t), 1, t.numel(), t.numel(), _p(out), _stream()), "amax")
    elif t.dim() == 2 and t.stride(1) == 1:
        check(lib.glf_amax(_p(t), t.shape[0], t.shape[1], t.stride(0), _p(out), _stream()), "amax")
    else:
        return None                      # the library measures the operand region itself
    try:
        t._glf_amax = (t._version, t.data_ptr(), out)
    except AttributeError:
        pass
    return out


_amax_pool = {}


def amax_slot(dev) -> Optional[torch.Tensor]:
    """A zeroed device float for a kernel that reports max|output| as a by-product (None unless f16x3 is
    active).  Slots come from a pre-zeroed pool per stream (one fill kernel per 4096 slots); a used-up pool stays
    alive through the slices that reference it."""
    if _PREC[0] < 2:
        return None
    key = torch.cuda.current_stream().cuda_stream          # the fill kernel and the users must share a stream
    pool = _amax_pool.get(key)
    if pool is None or pool[1] >= 4096 or pool[0].device != dev:
        pool = _amax_pool[key] = [zeros(4096, device=dev), 0]
    i = pool[1]
    pool[1] = i + 1
    return pool[0][i:i + 1]


_stats_pool = {}
_STATS_POOL_DOUBLES = 1 << 19


def stats_slot(c: int, dev) -> torch.Tensor:
    """A zeroed float64 [2, c] for a contraction's fused column statistics (glf_gemm_params.colstats), carved out of a
    per-stream pool that is zeroed in bulk (one fill per ~500 k doubles instead of one tiny fill per conv); a used-up pool
    stays alive through the slices that reference it."""
    key = torch.cuda.current_stream().cuda_stream
    need = 2 * c
    pool = _stats_pool.get(key)
    if pool is None or pool[1] + need > pool[0].numel() or pool[0].device != dev:
        pool = _stats_pool[key] = [zeros(max(_STATS_POOL_DOUBLES, need), dtype=torch.float64, device=dev), 0]
    i = pool[1]
    pool[1] = i + need
    return pool[0][i:i + need].view(2, c)


def bnbwd_slot(c: int, dev) -> torch.Tensor:
    """Zeroed scratch of glf_bn_bwd's two-launch form (fused_sums): 2 c doubles of sums followed by 2 c floats of maxima, carved out of
    the pooled, bulk-zeroed statistics buffer (stats_slot)."""
    return stats_slot((3 * c + 1) // 2, dev).view(-1)


_colmax_pool: dict = {}


def colmax_slot(c: int, dev) -> torch.Tensor:
    """A zeroed float32 [c] for a contraction's per-column maxima (glf_gemm_params.colmax), pooled like stats_slot."""
    key = torch.cuda.current_stream().cuda_stream
    pool = _colmax_pool.get(key)
    if pool is None or pool[1] + c > pool[0].numel() or pool[0].device != dev:
        pool = _colmax_pool[key] = [zeros(max(1 << 16, c), dtype=torch.float32, device=dev), 0]
    i = pool[1]
    pool[1] = i + c
    return pool[0][i:i + c]


def amax_bound(t: torch.Tensor, srcs: Sequence[Optional[torch.Tensor]], scale: float = 1.0, sum_: bool = False) -> None:
    """Attach to t an upper bound of its maximum derived from the maxima of the tensors it was made from (glf_amax_combine: one
    tiny launch per pair, no pass over the data): scale * max(srcs) or scale * sum(srcs).  Does nothing unless every source's
    maximum is known (t is then measured on first use, as before).  fp32 storage only: bf16 tensors carry no maxima."""
    if _PREC[0] < 2 or _is16(t):
        return
    ams = [getattr(x, "_glf_amax", None) for x in srcs]
    ams = [h[2] if (h is not None and h[0] == x._version and h[1] == x.data_ptr()) else None for h, x in zip(ams, srcs)]
    if not ams or any(a is None for a in ams):
        return
    out = amax_slot(t.device)
    if sum_:
        if len(ams) != 2:
            raise ValueError("amax_bound: sum_ takes exactly two sources")
        check(lib.glf_amax_combine(_p(ams[0]), _p(ams[1]), float(scale), 1, _p(out), _stream()), "amax_combine")
    else:
        for i in range(0, len(ams), 2):
            check(lib.glf_amax_combine(_p(ams[i]), _p(ams[i + 1]) if i + 1 < len(ams) else None, float(scale), 0, _p(out), _stream()), "amax_combine")
    set_amax(t, out)


def set_amax(t: torch.Tensor, amax: Optional[torch.Tensor]) -> None:
    """Attach a maximum produced as a by-product of the kernel that wrote t."""
    if amax is not None:
        t._glf_amax = (t._version, t.data_ptr(), amax)


def _tn_split(rows: int, m: int, n: int, ntaps: int, batch: int = 1) -> int:
    return conv_plan.tn_split(rows, m, n, ntaps, batch, _PREC[0])


# ----------------------------------------------------------------------------------------
# gradient slots: a parameter's gradient produced directly inside its all-reduce bucket (glfusion_amd.ddp)
# ----------------------------------------------------------------------------------------
_grad_slots = {}


def register_grad_slot(param: torch.Tensor, flat: torch.Tensor, offset: int) -> None:
    _grad_slots[id(param)] = [weakref.ref(param), flat, int(offset), False]


def unregister_grad_slots(params) -> None:
    for p in params:
        _grad_slots.pop(id(p), None)


def release_grad_slots(params) -> None:
    """End of a step: every slot may be handed out again."""
    for p in params:
        s = _grad_slots.get(id(p))
        if s is not None:
            s[3] = False


def grad_out(param: Optional[torch.Tensor], shape, device) -> torch.Tensor:
    """The tensor a backward kernel writes `param`'s gradient into: the parameter's slice of its all-reduce bucket when a
    GradAllReducer registered one and nobody took it yet this step (a parameter used several times per forward gets ONE
    in-bucket gradient -- autograd sums the others onto it), a fresh tensor otherwise.  The view is new every time, so
    autograd's AccumulateGrad can adopt it as .grad without a copy."""
    if param is not None and _grad_slots:
        s = _grad_slots.get(id(param))
        if s is not None and s[0]() is param and not s[3]:
            n = 1
            for d in shape:
                n *= int(d)
            if n == param.numel() and s[1].device == device and not torch.cuda.is_current_stream_capturing():
                s[3] = True
                return s[1][s[2]:s[2] + n].view(tuple(shape))
    return torch.empty(tuple(shape), dtype=torch.float32, device=device)


_ones_cache = {}


def _ones4(dev) -> torch.Tensor:
    t = _ones_cache.get(dev)
    if t is None:
        t = _ones_cache[dev] = torch.ones(4, dtype=torch.float32, device=dev)      # once per process
    return t


def colsum(dy2d: torch.Tensor, rows: int, c: int) -> torch.Tensor:
    """db[c] = sum_r dy[r][c] (bias gradients)."""
    db = torch.empty(c, dtype=torch.float32, device=dy2d.device)
    if c % 4 == 0:
        check(lib.glf_colsum(_p(dy2d), c, _p(db), rows, c, _p(_ws(rows, c, dy2d.device)), _stream()), "colsum")
    else:
        # tiny channel counts (the 5- and 1-channel heads): reduce with the TN contraction against a
        # broadcast 1.0 (row stride 0)
        one = _ones4(dy2d.device)
        gemm("tn", dy2d, one, db, M=c, N=1, K=rows, lda=c, ldb=0, ldc=1, split=_tn_split(rows, c, 1, 1))
    return db


def split_mode() -> bool:
    """True when contractions run on a split (bf16x6 / f16x3) kernel family, which has NT and TN forms only."""
    return _PREC[0] >= 1


def transpose2d(x: torch.Tensor, rows: int, cols: int, batch: int = 1) -> torch.Tensor:
    """[batch][rows][cols] -> [batch][cols][rows] (fresh tensor)."""
    out = torch.empty(batch * rows * cols, dtype=torch.float32, device=x.device)
    check(lib.glf_transpose2d(_p(x), _p(out), rows, cols, batch, _stream()), "transpose2d")
    return out


# Pre-split operands (split-fp16 precisions): an operand is split into its fp16 pieces ONCE, into a packed image of the same
# size and strides, instead of in the staging path of every tile of every launch that reads it.
PRESPLIT = os.environ.get("GLF_PRESPLIT", "1") != "0"
# An activation / gradient tensor is worth its split pass (one read + one write of the tensor) only if the contractions that
# read it re-split it often enough: the pass costs ~ rows x K x 8 bytes of HBM traffic, the NT kernel saves ~14 % and the
# weight-gradient kernel ~15 % of a time proportional to rows x K x (output columns x taps).  Break-even measured near
# columns x taps = 1000.  (Weights are always pre-split: once per update, cached.)
PRESPLIT_MIN_COLS = int(os.environ.get("GLF_PRESPLIT_MIN_COLS", "1024"))


def presplit_ok(t: torch.Tensor, amax: Optional[torch.Tensor]) -> bool:
    return (PRESPLIT and _PREC[0] >= 2 and amax is not None and t.dim() >= 1 and t.shape[-1] % 4 == 0
            and t.is_contiguous() and t.data_ptr() % 16 == 0)


def packed_of(t: torch.Tensor, amax: torch.Tensor) -> torch.Tensor:
    """The packed pre-split image of a contiguous fp32 tensor whose rows (last dim) hold a multiple of 4 elements: a tensor of
    the same shape (declared fp32, holding fp16 pairs) to pass as A / B with a_packed / b_packed and the SAME amax."""
    cols = t.shape[-1]
    out = torch.empty_like(t)
    check(lib.glf_split_f16_packed(_p(t), t.numel() // cols, cols, cols, _p(amax), _p(out), cols, _stream()), "split_f16_packed")
    return out


def weight_packed(layout: torch.Tensor, owner: torch.Tensor, tag: str, amax: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """packed_of(layout) for a dense weight layout derived from the parameter `owner`, made once per weight update (cached
    against the owner's version counter and the amax scalar it was scaled with).  None when not applicable."""
    if not presplit_ok(layout, amax):
        return None
    im, fresh = _wimage(owner, "pk:" + tag, WJ_PACK, layout, (layout.numel(), 0, 0), lambda: torch.empty_like(layout), amax)
    if fresh:
        cols = layout.shape[-1]
        check(lib.glf_split_f16_packed(_p(layout), layout.numel() // cols, cols, cols, _p(amax), _p(im.dst), cols, _stream()), "split_f16_packed")
    return im.dst


def packed_hit(t: torch.Tensor, amax: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The pre-split image already made of t (by an earlier consumer of this tensor object, or of another alias handed out by
    fan_out), or None."""
    hit = getattr(t, "_glf_packed", None)
    if hit is not None and hit[0] == t._version and hit[1] == t.data_ptr() and hit[2] is amax:
        pk, made_on = hit[3], (hit[4] if len(hit) > 4 else None)
        if made_on is not None:
            cur = torch.cuda.current_stream()
            if made_on.cuda_stream != cur.cuda_stream:   # a consumer on another side stream: order it behind the split pass
                cur.wait_stream(made_on)
                pk.record_stream(cur)
        return pk
    share = getattr(t, "_glf_pack_share", None)          # the aliases of one fan_out share one image
    if share is not None and share[0] is not None and share[0][0] == t.data_ptr() and share[0][1] is amax:
        pk, made_on = share[0][2], share[0][3]
        cur = torch.cuda.current_stream()
        if made_on.cuda_stream != cur.cuda_stream:       # the aliases' consumers may sit on different side streams
            cur.wait_stream(made_on)
            pk.record_stream(cur)
        return pk
    return None


# A pre-split image kept from the forward pass to the backward pass is a second copy of that activation.  At C2 that is 33 GB
# on top of 56 GB; at the 5-view 224^2 shape it took the step from 180 GB to 264 GB of the 288 GB and the allocator started
# thrashing (1.16 s -> 4.0 s per step).  So images are RETAINED (on the tensor object, for the weight gradient) only while the
# device has room: while the caching allocator has RESERVED less than this fraction of the device memory (reserved, not
# allocated: with one block pool per stream the reserved figure runs far ahead -- at that shape 205 GB allocated already
# thrashed).  Above it an image lives for the launches of one autograd node: 1.02 s per step there, against 1.12 s without
# any pre-split.
PRESPLIT_KEEP_FRAC = float(os.environ.get("GLF_PRESPLIT_KEEP_FRAC", "0.5"))
PRESPLIT_OFF_FRAC = float(os.environ.get("GLF_PRESPLIT_OFF_FRAC", "0.6"))
_dev_total = {}
_retain_off = {}
_retain_step = {}


def retain_ok(dev) -> bool:
    """Retained images sit in memory across the peak of the step (end of forward), so the decision cannot be made tensor by
    tensor: once the allocator has been seen above PRESPLIT_OFF_FRAC of the device, retention is off for the rest of the
    process (the workload does not fit with second copies; the first step pays for finding out)."""
    hit = _retain_step.get(dev)
    if hit is not None:                       # decided at the first pack of this step (begin_step clears it): no allocator
        return hit                            # queries per conv, and the step does not change its mind half-way
    tot = _dev_total.get(dev)
    if tot is None:
        tot = _dev_total[dev] = torch.cuda.get_device_properties(dev).total_memory
    off = _retain_off.get(dev, 0)
    if off:
        if off == 1 and torch.cuda.memory_allocated(dev) < 0.3 * tot and not torch.cuda.is_current_stream_capturing():
            # first pack of a later step: the images retained before the switch are gone -- hand the pools they inflated
            # back to the device once (a later step needs less than the one that found out)
            torch.cuda.empty_cache()
            _retain_off[dev] = 2
        _retain_step[dev] = False
        return False
    r = torch.cuda.memory_reserved(dev)
    if r > PRESPLIT_OFF_FRAC * tot:
        _retain_off[dev] = 1                  # this step keeps what it already retained; the next ones retain nothing
        _retain_step[dev] = False
        return False
    ok = r < PRESPLIT_KEEP_FRAC * tot
    if ok:
        _retain_step[dev] = True              # a "no" below the off threshold is re-examined at the next pack
    return ok


def act_packed(t: torch.Tensor, amax: Optional[torch.Tensor], retain: Optional[bool] = None) -> Optional[torch.Tensor]:
    """packed_of(t) for an activation / gradient tensor, remembered on the tensor object (like its amax) so that every
    contraction that reads it -- a conv input in the forward of each consumer and again in its weight gradient, an output
    gradient in dgrad and wgrad -- shares one split pass.  retain: keep the image alive with t (default: while the device
    has memory to spare, see retain_ok; gradients pass True: they die with their autograd node).  None when not applicable."""
    if not presplit_ok(t, amax):
        return None
    pk = packed_hit(t, amax)
    if pk is not None:
        return pk
    pk = packed_of(t, amax)
    if retain is None:
        retain = retain_ok(t.device)
    if retain:
        try:
            t._glf_packed = (t._version, t.data_ptr(), amax, pk, torch.cuda.current_stream() if STREAMS else None)
        except AttributeError:
            pass
        share = getattr(t, "_glf_pack_share", None)
        if share is not None:
            share[0] = (t.data_ptr(), amax, pk, torch.cuda.current_stream())
    return pk


def act_packed_colsum(t: torch.Tensor, amax: Optional[torch.Tensor], rows: int, cols: int):
    """act_packed(t, amax, True) for a gradient [rows, cols] whose column sums are wanted too (a bias gradient): ONE pass writes the
    image and the sums (glf_split_f16_packed_colsum).  -> (image, sums); (None, None) where no image is made here -- not
    applicable, or one exists already -- and the caller takes act_packed / colsum."""
    if not presplit_ok(t, amax) or packed_hit(t, amax) is not None:
        return None, None
    pk = torch.empty_like(t)
    db = torch.empty(cols, dtype=torch.float32, device=t.device)
    check(lib.glf_split_f16_packed_colsum(_p(t), rows, cols, cols, _p(amax), _p(pk), cols, _p(db), _p(_ws(rows, cols, t.device)), _stream()),
          "split_f16_packed_colsum")
    try:
        t._glf_packed = (t._version, t.data_ptr(), amax, pk, torch.cuda.current_stream() if STREAMS else None)
    except AttributeError:
        pass
    return pk, db


def nt_presplit_ok(K: int, lda: int, ldb: int) -> bool:
    """Mirror of the library's eligibility test for the aligned split-fp16 NT kernel (gemm_f16s.hip f16s_rows_ok)."""
    return _PREC[0] >= 2 and K % 32 == 0 and 32 <= K <= (1 << 18) and lda % 4 == 0 and ldb % 4 == 0


def tn_presplit_ok(M: int, N: int, lda: int, ldb: int) -> bool:
    """Same for the TN kernel (f16s_tn_ok)."""
    return _PREC[0] >= 2 and M % 4 == 0 and N % 4 == 0 and 4 <= M <= (1 << 18) and 4 <= N <= (1 << 18) and lda % 4 == 0 and ldb % 4 == 0


def pick(t: torch.Tensor, packed: Optional[torch.Tensor], ok: bool):
    """(operand, packed flag) for a gemm() call."""
    return (packed, True) if (ok and packed is not None) else (t, False)


def weight_T(w2d: torch.Tensor, owner: torch.Tensor) -> torch.Tensor:
    """Transposed copy [cols][rows] of a 2-D weight view, cached against the owning parameter's version."""
    rows, cols = w2d.shape
    src = _contig(w2d)
    im, fresh = _wimage(owner, "T2", WJ_TRANSPOSE, src, (rows, cols, 0),
                        lambda: torch.empty(cols, rows, dtype=torch.float32, device=owner.device))
    if fresh:
        check(lib.glf_transpose2d(_p(src), _p(im.dst), rows, cols, 1, _stream()), "transpose2d")
    return im.dst


def tap_major_T(weight: torch.Tensor) -> torch.Tensor:
    """[tap][Cin][Cout] re-layout (dgrad as an NT contraction), cached like tap_major."""
    co, ci, kh, kw = weight.shape
    src = _contig(weight.detach())
    taps = kh * kw
    mk = lambda: torch.empty(taps, ci, co, dtype=torch.float32, device=weight.device)
    if taps == 1:                      # a plain transpose [co][ci] -> [ci][co]
        im, fresh = _wimage(weight, "tapT", WJ_TRANSPOSE, src, (co, ci, 0), mk)
        if fresh:
            check(lib.glf_transpose2d(_p(src), _p(im.dst), co, ci, 1, _stream()), "transpose2d")
        return im.dst
    im, fresh = _wimage(weight, "tapT", WJ_TAP_MAJOR_T, src, (co, ci, taps), mk)
    if fresh:
        check(lib.glf_oihw_to_tap_major_t(_p(src), _p(im.dst), co, ci, taps, _stream()), "oihw_to_tap_major_t")
    return im.dst


def tap_major(weight: torch.Tensor) -> torch.Tensor:
    """OIHW -> [tap][Cout][Cin], recomputed only when the parameter changes (a view for 1x1 weights)."""
    co, ci, kh, kw = weight.shape
    if kh * kw == 1:
        return _contig(weight.detach()).view(1, co, ci)
    src = _contig(weight.detach())
    im, fresh = _wimage(weight, "tap", WJ_TAP_MAJOR, src, (co, ci, kh * kw),
                        lambda: torch.empty(kh * kw, co, ci, dtype=torch.float32, device=weight.device))
    if fresh:
        check(lib.glf_oihw_to_tap_major(_p(src), _p(im.dst), co, ci, kh * kw, _stream()), "oihw_to_tap_major")
    return im.dst


# ----------------------------------------------------------------------------------------
# conv2d (NHWC, implicit GEMM)
# ----------------------------------------------------------------------------------------
def tn_oihw_ok(cin: int, taps: int, dw: torch.Tensor) -> bool:
    """True when glf_gemm_tn's second stage can store the parameter-shaped gradient `dw` itself (glf_gemm_params.c_oihw): a
    multi-tap kernel of at most TN_OIHW_MAX_TAPS taps, Cin % 4 == 0 and a 16-byte aligned destination (a bucket slot may start
    at any float)."""
    return 1 < taps <= TN_OIHW_MAX_TAPS and cin % 4 == 0 and dw.data_ptr() % 16 == 0 and dw.is_contiguous()


def _conv_wgrad(weight, wshape, x, x_packed, da, lda: int, pa: bool, am_dy, pl, foreign=None, out=None):
    """The weight gradient of a convolution from its output gradient `da` (row stride lda; pa: a packed pre-split image scaled by
    am_dy) as pl = conv_plan.plan("wgrad", ...) lays it out: the parameter-shaped gradient (in its all-reduce bucket slot where
    one is registered).  Taps outside pl.mask receive zeros, except foreign = (tap, src [Cout][Cin], row stride): that tap, not in
    the mask, is copied from src.  A multi-tap gradient is stored in parameter layout by the reduction itself (tn_oihw_ok): no
    tap-major intermediate, no zero fill, no re-layout pass; an empty mask then launches that store alone.
    out: the destination the caller already took with grad_out()."""
    cout, cin, taps, full = pl.M, pl.N, pl.taps, not pl.zero_fill
    dw = (out if out is not None else grad_out(weight, wshape, x.device)) if taps > 1 else None
    fused = taps > 1 and tn_oihw_ok(cin, taps, dw)
    if fused:
        dwt = dw
    elif taps == 1 and full:                                   # a 1x1 weight's gradient is the contraction's output
        dwt = out.view(1, cout, cin) if out is not None else grad_out(weight, (1, cout, cin), x.device)
    else:
        dwt = (torch.empty if full else zeros)(taps, cout, cin, dtype=torch.float32, device=x.device)
    ok = tn_presplit_ok(cout, cin, lda, cin)
    am_x = x_packed[1] if x_packed is not None else amax_of(x)
    xb, pb = pick(x, x_packed[0] if x_packed is not None else None, ok)        # x: the image the forward made, if any
    if pl.kept or fused:
        gemm("tn", da, xb, dwt, M=cout, N=cin, K=pl.K, lda=lda, ldb=cin, ldc=cin, taps=taps, mask=pl.mask, tap_stride_b=cout * cin,
             gather=pl.gather, geo=pl.geo, split=pl.split, rect=pl.rect, amax_a=am_dy, amax_b=am_x, a_packed=pa, b_packed=pb,
             oihw=fused, foreign=foreign if fused else None)
    if fused:
        return dw
    if taps == 1:
        return dwt.view(wshape)
    if foreign is not None:                # (a destination the fused store cannot take: the tap joins the tap-major image)
        check(lib.glf_copy_frames(_p(foreign[1]), foreign[2], _p(dwt[foreign[0]]), cin, cout, cin, _stream()), "conv_wgrad(foreign tap)")
    check(lib.glf_tap_major_to_oihw(_p(dwt), _p(dw), cout, cin, taps, _stream()), "tap_major_to_oihw")
    return dw


class Conv2dFn(Function):
    """F.conv2d on [N,H,W,Cin] with torch-layout weights [Cout,Cin,kh,kw] (groups = 1)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride: int, pad: int, dil: int, colstats=None):
        _chk(x, "conv input"); _chk(weight, "conv weight")
        x = _contig(x)
        n, h, w, cin = x.shape
        cout, cin_w, kh, kw = weight.shape
        if cin_w != cin:
            raise RuntimeError(f"conv2d: input has {cin} channels, weight expects {cin_w}")
        geom = (n, h, w, cin, cout, kh, kw, stride, pad, dil)
        pl = conv_plan.plan("fwd", geom, _PREC[0], bias=bias is not None)
        ho, wo, taps, plain, mask, rect = pl.ho, pl.wo, pl.taps, pl.plain, pl.mask, pl.rect
        if ho <= 0 or wo <= 0:
            raise RuntimeError("conv2d: empty output")
        wt = tap_major(weight)
        y = torch.empty(n, ho, wo, cout, dtype=torch.float32, device=x.device)
        if pl.zero_fill:
            zero_(y)
            if colstats is not None:
                raise RuntimeError("conv2d: fused column statistics are not available for a conv evaluated as per-tap rectangles")
        am_w, am_x = amax_of(weight), amax_of(x)
        x_pk = packed_only(x)                # the producing BatchNorm wrote the activation as a packed image (no fp32 form exists)
        # <= 64 output rows (the ASPP pooled branch: one row per frame): glf_gemm_nt's skinny kernel takes plain fp32 operands
        skinny = plain and pl.M <= 64 and cout >= 64 and cin % 16 == 0 and not x_pk and colstats is None
        ok = nt_presplit_ok(cin, cin, cin) and not skinny
        if x_pk and not (ok and am_x is not None and takes_packed_input(weight)):
            raise RuntimeError("glfusion_amd: a packed-only activation reached a convolution that cannot consume it")
        ok_x = ok and (cout * pl.kept >= PRESPLIT_MIN_COLS or packed_hit(x, am_x) is not None)
        xa, pa = (x, True) if x_pk else pick(x, act_packed(x, am_x) if ok_x else None, ok_x)
        wb, pb = pick(wt, weight_packed(wt, weight, "w", am_w) if ok else None, ok)
        # exact fp32 (the strict-precision leg): per-tap rectangles ONE TAP PER LAUNCH.  In one launch the taps of an output pixel meet in
        # float atomics in whatever order the workgroups finish; the order-dependent last bits of the ASPP outputs are harmless in the
        # forward pass (loss to 3e-8) and came back from this model's backward pass (BatchNorm over the N per-frame averages of the
        # pooled branch) as 2-8e-3 run-to-run changes of whole gradient tensors (profiles/r04_exact_leg_spread.txt).  Tap after tap every
        # element gets its addends in tap order: reproducible, and the rectangles' short fp32 chains are kept (a dense evaluation is a
        # 9 K-long chain and moved the train-mode logits past 1e-4).
        masks = [1 << t_ for t_ in range(taps) if (mask >> t_) & 1] if (rect and _PREC[0] == 0) else [mask]
        for mk in masks:
            gemm("nt", xa, wb, y, M=pl.M, N=cout, K=cin, lda=cin, ldb=cin, ldc=cout, bias=bias,
                 taps=taps, mask=mk, tap_stride_b=cout * cin, gather=pl.gather, geo=pl.geo, rect=rect,
                 amax_a=am_x, amax_b=am_w, colstats=colstats, colmax=getattr(colstats, "_glf_colmax", None), a_packed=pa, b_packed=pb)
        ctx.save_for_backward(x, wt)
        ctx.x_packed = (xa, am_x) if (pa and (x_pk or packed_hit(x, am_x) is not None)) else None      # retained: the weight gradient reads the same image
        ctx.weight_ref = weight            # for the cached [tap][Cin][Cout] layout of the split-bf16 dgrad
        ctx.cfg = (geom, bias is not None, tuple(weight.shape))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, wt = ctx.saved_tensors
        geom, has_bias, wshape = ctx.cfg
        cin, cout = geom[3], geom[4]
        dy = _contig(dy)
        dx = dw = db = None
        am_dy, am_w = amax_of(dy), amax_of(ctx.weight_ref)
        dy_pk = packed_only(dy)              # BatchNorm backward wrote the gradient as a packed pre-split image (no fp32 form exists)
        if dy_pk and (has_bias or am_dy is None or not (split_mode() and cout % 32 == 0)):
            raise RuntimeError("glfusion_amd: a packed-only gradient reached a convolution that cannot consume it")
        def dgrad():
            pl = conv_plan.plan("dgrad", geom, _PREC[0])
            if pl.mask == 0:
                return zeros(x.shape, device=x.device)
            dx = zeros(x.shape, device=x.device) if pl.zero_fill else torch.empty_like(x)
            if split_mode() and cout % 32 == 0:
                # dgrad as NT on the split-bf16 kernels: B_tap[n = ci][k = co]
                wT = tap_major_T(ctx.weight_ref)
                ok = nt_presplit_ok(cout, cout, cout)
                ok_dy = ok and cin * pl.kept >= PRESPLIT_MIN_COLS
                da, pa = (dy, True) if dy_pk else pick(dy, act_packed(dy, am_dy, True) if ok_dy else None, ok_dy)
                wb, pb = pick(wT, weight_packed(wT, ctx.weight_ref, "wT", am_w) if ok else None, ok)
                gemm("nt", da, wb, dx, M=pl.M, N=cin, K=cout, lda=cout, ldb=cout, ldc=cin, taps=pl.taps, mask=pl.mask,
                     tap_stride_b=cout * cin, gather=pl.gather, geo=pl.geo, rect=pl.rect, amax_a=am_dy, amax_b=am_w, a_packed=pa, b_packed=pb)
            else:
                gemm("nn", dy, wt, dx, M=pl.M, N=cin, K=cout, lda=cout, ldb=cin, ldc=cin, taps=pl.taps, mask=pl.mask,
                     tap_stride_b=cout * cin, gather=pl.gather, geo=pl.geo, rect=pl.rect)
            return dx

        def wgrad():
            pl = conv_plan.plan("wgrad", geom, _PREC[0])
            ok = tn_presplit_ok(cout, cin, cout, cin)
            # dy: the image dgrad made (or one worth making for this kernel alone)
            ok_dy = ok and (packed_hit(dy, am_dy) is not None or cin * pl.kept >= PRESPLIT_MIN_COLS)
            da, pa = (dy, True) if dy_pk else pick(dy, act_packed(dy, am_dy, True) if ok_dy else None, ok_dy)
            return _conv_wgrad(ctx.weight_ref, wshape, x, ctx.x_packed, da, cout, pa, am_dy, pl)

        if ctx.needs_input_grad[0]:
            dx = dgrad()
        if ctx.needs_input_grad[1]:
            dw = wgrad()
        if has_bias and ctx.needs_input_grad[2]:
            db = colsum(dy, dy.numel() // cout, cout)
        return dx, dw, db, None, None, None, None


def conv2d(x, weight, bias=None, stride: int = 1, pad: int = 0, dil: int = 1, colstats=None):
    if _is16(x):
        from . import ops16
        return ops16.conv2d(x, weight, bias, stride, pad, dil, colstats)
    return Conv2dFn.apply(x, weight, bias, stride, pad, dil, colstats)


def conv_stats_fusable(weight, stride: int, pad: int, dil: int, h: int, w: int, dtype=None) -> bool:
    """True when conv2d(..., colstats=) is honoured: the forward plan's colstats_ok (f16x3 kernels, Cin % 32 == 0, Cout % 4 == 0, not
    a conv that runs as per-tap rectangles with atomics -- ASPP rate 12 / 24; 16-bit storage: Cin % 64 == 0 and Cout % 64 == 0)
    for a non-empty output and, under 16-bit storage, a bf16 input."""
    if _S16[0] and dtype != torch.bfloat16:
        return False
    cout, cin, kh, kw = weight.shape
    pl = conv_plan.plan("fwd", (1, h, w, cin, cout, kh, kw, stride, pad, dil), conv_plan.S16 if _S16[0] else _PREC[0])
    return pl.colstats_ok and pl.ho > 0 and pl.wo > 0


# ----------------------------------------------------------------------------------------
# ASPP conv branches: the centre taps as ONE contraction (split-fp16 precisions)
# ----------------------------------------------------------------------------------------
# The 1x1 branch and the centre taps of the 3x3 "same" branches (pad == dil: the centre tap is in range for every pixel) are
# full-map products over the same input.  Stacked, they are one plain launch with N = k Cout forward and one with K = k Cout in
# dgrad, at the shapes the big projections run at; the off-centre taps of a branch keep the launch the branch would use alone
# (conv_plan.plan(..., keep=~CENTRE_TAP)) and ADD into what the stacked launch stored.  The four BatchNorm backward passes write
# their gradients as column slices of one packed image under one scale (_GradGroup), and the head's input gradient is one tensor
# where there were four plus a sum.
ASPP_CENTRE = os.environ.get("GLF_ASPP_CENTRE", "1") != "0"
# the centre taps' WEIGHT gradients as one stacked contraction too (0: one contraction per branch, centre tap included)
ASPP_CENTRE_WGRAD = os.environ.get("GLF_ASPP_CENTRE_WGRAD", "1") != "0"
_centre_cache = {}


def _tap_slab_into(src: torch.Tensor, taps: int, tap: int, dst: torch.Tensor, cout: int, cin: int, what: str) -> None:
    """dst [Cout][Cin] = tap `tap` of the contiguous OIHW weight src, outside the multi-tensor refresh (a new or stale image):
    the strided gather the image's GLF_WJ_COPY job does.  Not through tap_major(): that would register the whole tap-major
    image of the weight, 9 Cout Cin floats recomputed with every update, for a head whose launches read none of it."""
    if taps == 1:
        check(lib.glf_copy_frames(_p(src), cout * cin, _p(dst), cout * cin, 1, cout * cin, _stream()), what)
    else:
        dst.copy_(src.view(cout, cin, taps)[:, :, tap])


def aspp_centre_weights(weights) -> torch.Tensor:
    """Wc [k Cout][Cin]: the 1x1 weight and the centre taps of the 3x3 weights stacked by rows, bit-identical to slicing the
    parameters.  Like fusion._qkv_weights: the buffer lives as long as the first weight, every row block is a registered weight
    image of its parameter (GLF_WJ_COPY, for a 3x3 weight its strided-gather form), and Wc carries the combined version stamp of its sources for the
    images derived from IT (maximum, transpose, packed forms)."""
    w0 = weights[0]
    cout, cin, k = w0.shape[0], w0.shape[1], len(weights)
    key = id(w0)
    hit = _centre_cache.get(key)
    if (hit is None or hit[0]() is not w0 or hit[1].device != w0.device or tuple(hit[1].shape) != (k * cout, cin)
            or any(r() is not t for r, t in zip(hit[1]._glf_sources, weights))):
        Wc = torch.empty(k * cout, cin, dtype=torch.float32, device=w0.device)
        refs = [weakref.ref(t) for t in weights]
        Wc._glf_version_fn = lambda refs=refs: tuple((r()._version, r().data_ptr()) if r() is not None else None for r in refs)
        Wc._glf_sources = refs
        hit = _centre_cache[key] = (weakref.ref(w0, lambda _r, k_=key: _centre_cache.pop(k_, None)), Wc)
    Wc = hit[1]
    for i, t in enumerate(weights):
        taps = t.shape[2] * t.shape[3]
        src, dst = _contig(t.detach()), Wc[i * cout:(i + 1) * cout]
        kind, dims = WJ_COPY, (cout * cin, 0, 0) if taps == 1 else (cout * cin, taps, taps // 2)
        im, fresh = _wimage(t, "centre", kind, src, dims, lambda dst=dst: dst)
        if im.dst.data_ptr() != dst.data_ptr():       # the stacked buffer was re-created: re-register
            _registry(t.device).drop(im.key)
            im, fresh = _wimage(t, "centre", kind, src, dims, lambda dst=dst: dst)
        if fresh:
            _tap_slab_into(src, taps, taps // 2, im.dst, cout, cin, "aspp_centre_weights")
    return Wc


# The head's input gradient as ONE launch (glf_gemm_params.nseg): the stacked centre contraction G Wc^T extended by one extra
# segment per kept off-centre tap of the dilated branches -- every element of dx stored once, where the off-centre taps used
# to be region-mode launches that read dx back and added to it.  0: those launches.
ASPP_DGRAD_ONE = os.environ.get("GLF_ASPP_DGRAD_ONE", "1") != "0"
_dgrad_cache = {}


def aspp_dgrad_segments(dils, h: int, w: int, cout: int):
    """[(branch, tap, oy, ox, acol)] of the kept off-centre taps of the dilated branches on an h x w map, branch by branch in tap
    order: the tap reads the gradient pixel (y + oy, x + ox) of column block acol of the stacked gradient image."""
    segs = []
    for i, d in enumerate(dils, start=1):
        off = tap_mask(2, h, w, h, w, 3, 3, 1, d, d) & ~CENTRE_TAP
        for t in range(9):
            if (off >> t) & 1:
                ky, kx = divmod(t, 3)
                segs.append((i, t, (1 - ky) * d, (1 - kx) * d, i * cout))
    return segs


def aspp_dgrad_weights(weights, segs) -> torch.Tensor:
    """Wd [(k + nseg) Cout][Cin]: the rows of aspp_centre_weights (Wc), then the tap slab [Cout][Cin] of every segment in
    aspp_dgrad_segments order.  Built and cached like Wc (GLF_WJ_COPY jobs of the multi-tensor refresh, the combined version stamp
    of its sources for the images derived from it); one buffer per set of kept taps, which depends on the map's size."""
    w0 = weights[0]
    cout, cin, k = w0.shape[0], w0.shape[1], len(weights)
    blocks = [(i, 4 if weights[i].shape[2] * weights[i].shape[3] == 9 else 0) for i in range(k)] + [(i, t) for i, t, _, _, _ in segs]
    sk = ",".join("%d.%d" % b for b in blocks[k:])
    per = _dgrad_cache.get(id(w0))
    if per is None or per[0]() is not w0:
        per = _dgrad_cache[id(w0)] = (weakref.ref(w0, lambda _r, k_=id(w0): _dgrad_cache.pop(k_, None)), {})
    Wd = per[1].get(sk)
    if (Wd is None or Wd.device != w0.device or tuple(Wd.shape) != (len(blocks) * cout, cin)
            or any(r() is not t for r, t in zip(Wd._glf_sources, weights))):
        Wd = torch.empty(len(blocks) * cout, cin, dtype=torch.float32, device=w0.device)
        refs = [weakref.ref(t) for t in weights]
        Wd._glf_version_fn = lambda refs=refs: tuple((r()._version, r().data_ptr()) if r() is not None else None for r in refs)
        Wd._glf_sources = refs
        per[1][sk] = Wd
    for b, (i, tap) in enumerate(blocks):
        t = weights[i]
        taps = t.shape[2] * t.shape[3]
        src, dst = _contig(t.detach()), Wd[b * cout:(b + 1) * cout]
        kind, dims = WJ_COPY, (cout * cin, 0, 0) if taps == 1 else (cout * cin, taps, tap)
        tag = "dgrad1:%s:%d" % (sk, b)
        im, fresh = _wimage(t, tag, kind, src, dims, lambda dst=dst: dst)
        if im.dst.data_ptr() != dst.data_ptr():       # the stacked buffer was re-created: re-register
            _registry(t.device).drop(im.key)
            im, fresh = _wimage(t, tag, kind, src, dims, lambda dst=dst: dst)
        if fresh:
            _tap_slab_into(src, taps, tap, im.dst, cout, cin, "aspp_dgrad_weights")
    return Wd


def _aspp_dgrad_one(G, am_g, weights, dils, dx, slot, n: int, h: int, w: int, cin: int, cout: int) -> bool:
    """dx = G Wd^T in one segmented launch; False when this head does not take that route (the caller runs the stacked and the
    per-branch launches)."""
    k = len(weights)
    ldu = k * cout
    segs = aspp_dgrad_segments(dils, h, w, cout)
    if not ASPP_DGRAD_ONE or _PREC[0] not in (2, 3) or not segs or len(segs) > SEG_MAX or cout % 32 != 0 or ldu % 32 != 0:
        return False
    Wd = aspp_dgrad_weights(weights, segs)
    am_wd = amax_of(Wd)
    WdT = weight_T(Wd, Wd)
    wb = weight_packed(WdT, Wd, "wT", am_wd)
    if wb is None:
        return False
    rows, ldb = n * h * w, Wd.shape[0]
    # executed work: the centre slices of every pixel plus the (pixel, in-range segment) pairs; dense: what the stacked launch
    # and the off-centre launches it replaces reported together (every tap of those branches, padding included)
    pairs = sum(max(0, h - abs(oy)) * max(0, w - abs(ox)) for _, _, oy, ox, _ in segs)
    executed = 2.0 * cin * cout * (rows * k + n * pairs)
    dense = 2.0 * rows * cin * (ldu + 9 * cout * len({i for i, _, _, _, _ in segs}))
    return gemm("nt", G, wb, dx, M=rows, N=cin, K=ldu, lda=ldu, ldb=ldb, ldc=cin, geo=(n, h, w, h, w, 1, 1, 1, 0, 1),
                amax_a=am_g, amax_b=am_wd, amax_c=slot, a_packed=True, b_packed=True,
                seg=(cout, [(oy, ox, acol) for _, _, oy, ox, acol in segs], dense, executed))


# The head's FORWARD as one launch (glf_gemm_nt_seg_cols): the stacked centre contraction x Wc^T extended by one segment per kept
# off-centre tap, each adding to its own branch's columns only -- every element of U stored once, with final column statistics
# for every branch, where the rate-12 / 24 taps used to be per-tap rectangles that add into U with float atomics and leave their
# BatchNorms to reduce their own statistics.  0: those launches.
ASPP_FWD_ONE = os.environ.get("GLF_ASPP_FWD_ONE", "1") != "0"
COL_TILE = 128                         # column groups of a segmented launch are whole column tiles of the NT kernel


def aspp_fwd_segments(dils, h: int, w: int, cout: int):
    """[(branch, tap, oy, ox, first column)] of the kept off-centre taps of the dilated branches on an h x w map, branch by
    branch in tap order: the tap reads the input pixel (y + oy, x + ox) and adds to the columns [first, first + cout) of U."""
    segs = []
    for i, d in enumerate(dils, start=1):
        off = tap_mask(1, h, w, h, w, 3, 3, 1, d, d) & ~CENTRE_TAP
        for t in range(9):
            if (off >> t) & 1:
                ky, kx = divmod(t, 3)
                segs.append((i, t, (ky - 1) * d, (kx - 1) * d, i * cout))
    return segs


def aspp_fwd_weights(weights, segs) -> torch.Tensor:
    """Wf [(k + nseg) Cout][Cin]: the rows of aspp_centre_weights (Wc), then the tap slab [Cout][Cin] of every segment in
    aspp_fwd_segments order -- each branch's taps in row blocks of their own, reached through a B offset per segment
    (aspp_fwd_cols), not a dense [k Cout][Cin + nseg Cin] image that would be 3/4 unused.  The same row blocks in the same order
    as aspp_dgrad_weights' (a 3x3 pad == dil conv keeps the same taps in both directions): ONE buffer, one set of GLF_WJ_COPY
    jobs and one maximum serve the head's forward and its input gradient; the forward adds its packed form."""
    return aspp_dgrad_weights(weights, segs)


def aspp_fwd_cols(segs, k: int, cout: int, cin: int):
    """[(first column, columns, B offset)] per segment for gemm(seg_cols=): segment s is row block k + s of aspp_fwd_weights'
    image, so its slice for column c of its branch starts (k + s) Cout - first column rows behind the start of row c."""
    return [(col0, cout, ((k + s) * cout - col0) * cin) for s, (_, _, _, _, col0) in enumerate(segs)]


def _aspp_fwd_one(x, am_x, weights, dils, U, sums, n: int, h: int, w: int, cin: int, cout: int):
    """U = x Wf^T in one segmented launch with column groups; the packed x it read, or None when this head does not take that
    route (nothing ran: the caller makes the stacked and the per-branch launches).  Under engine.StepGraph the first launch of a
    plan, which allocates and copies its device table, happens in the eager warm-up steps, as for the input gradient's launch."""
    k = len(weights)
    ldu = k * cout
    if not ASPP_FWD_ONE or _PREC[0] not in (2, 3) or cout % COL_TILE != 0 or not nt_presplit_ok(cin, cin, cin):
        return None
    segs = aspp_fwd_segments(dils, h, w, cout)
    if not segs or len(segs) > SEG_MAX:
        return None
    Wf = aspp_fwd_weights(weights, segs)
    am_wf = amax_of(Wf)
    wb = weight_packed(Wf, Wf, "w", am_wf)
    xa = act_packed(x, am_x)
    if wb is None or xa is None:
        return None
    rows = n * h * w
    # executed work: the K columns of every pixel plus the (pixel, in-range segment) pairs; dense: what the stacked launch and the
    # off-centre launches it replaces reported together (every tap of those branches, padding included)
    pairs = sum(max(0, h - abs(oy)) * max(0, w - abs(ox)) for _, _, oy, ox, _ in segs)
    executed = 2.0 * cin * cout * (rows * k + n * pairs)
    dense = 2.0 * rows * cin * (ldu + 9 * cout * len({i for i, _, _, _, _ in segs}))
    ok = gemm("nt", xa, wb, U, M=rows, N=ldu, K=cin, lda=cin, ldb=cin, ldc=ldu, geo=(n, h, w, h, w, 1, 1, 1, 0, 1),
              amax_a=am_x, amax_b=am_wf, colstats=sums, a_packed=True, b_packed=True,
              seg=(cin, [(oy, ox, 0) for _, _, oy, ox, _ in segs], dense, executed), seg_cols=aspp_fwd_cols(segs, k, cout, cin))
    return xa if ok else None


def aspp_centre_ok(x: torch.Tensor, convs) -> bool:
    """True when AsppCentreFn takes the conv branches `convs` (modules with .weight/.bias/.stride/.padding/.dilation) of an
    ASPP over x: a split-fp16 precision with pre-split operands and packed gradients, one 1x1 conv followed by 3x3 stride-1
    pad == dil convs of equal Cin / Cout, no biases, Cin % 32 == 0 and Cout % 32 == 0.  Cout % 32 and not % 4: the gradient
    image G exists in packed form only, and the off-centre dgrad launches contract over K = Cout of one column slice of it on
    the aligned NT kernel, whose K step is 32 (nt_presplit_ok; the same bound takes_packed_grad sets for a single conv)."""
    if not ASPP_CENTRE or _PREC[0] < 2 or _S16[0] or _is16(x) or packed_only(x) or x.dim() != 4 or len(convs) < 2:
        return False
    w0 = convs[0].weight
    cout, cin = w0.shape[0], w0.shape[1]
    if cin != x.shape[-1] or cin % 32 != 0 or cout % 32 != 0 or not takes_packed_grad(w0) or not nt_presplit_ok(len(convs) * cout, 4, 4):
        return False
    for i, cv in enumerate(convs):
        k, d = (1, 1) if i == 0 else (3, int(cv.dilation[0]))
        pad = 0 if i == 0 else d
        if (tuple(cv.weight.shape) != (cout, cin, k, k) or cv.bias is not None or tuple(cv.stride) != (1, 1) or cv.groups != 1
                or tuple(cv.padding) != (pad, pad) or tuple(cv.dilation) != (d, d) or not cv.weight.is_contiguous()):
            return False
    return True


class _GradGroup:
    """The packed image G [rows][k Cout] that the BatchNorm layers behind AsppCentreFn's k outputs write their input gradients
    into, column slice by column slice, under ONE power-of-two scale: every layer's reduction raises its bound of max|dx| into
    the shared slot (glf_bn_bwd packed_dx = 2) and keeps its apply pass (packed_dx = 3) back until the last layer's bound is in.
    The channel sums an apply pass needs stay in `sums`, which the group owns: dgamma / dbeta are handed to autograd as soon as
    a layer's reduction is enqueued, and a gradient all-reduce may sum them over ranks before the held-back pass runs."""

    def __init__(self, k: int, cout: int):
        self.k, self.cout = k, cout
        self.G = self.amax = self.sums = None
        self.pending, self.seen = [], 0

    def bn_backward(self, i, dy, lddy, dy2, lddy2, x, ldx, y, ldy, mean, invstd, gamma, beta, dgamma, dbeta, rows, c, relu, training, has_mask):
        if not (PACKED_GRADS and _PREC[0] >= 2 and c == self.cout):
            raise RuntimeError("glfusion_amd: the stacked ASPP gradient image needs packed gradients under a split-fp16 precision")
        dev = dy.device
        if self.G is None:
            self.G = torch.empty(rows, self.k * c, dtype=torch.float32, device=dev)
            self.sums = torch.empty(self.k, 2 * c, dtype=torch.float32, device=dev)
        if self.seen == 0:
            self.amax = amax_slot(dev)           # a round of its own for every backward pass (retain_graph): the bound starts at zero
        ld = self.k * c
        keep = self.sums[i]
        dx = self.G.view(tuple(x.shape[:-1]) + (ld,))[..., i * c:(i + 1) * c]
        ws = _ws(rows, c, dev)

        def call(phase: int, dg=None, db=None):      # (the held-back pass keeps no reference to dgamma / dbeta: autograd adopts them)
            check(lib.glf_bn_bwd(_p(dy), lddy, _p(x), ldx, None if has_mask else _p(y), ldy, _p(mean), _p(invstd), _p(gamma), _p(beta),
                                 _p(dx), ld, None, c, _p(dg), _p(db), rows, c, int(relu), int(training), _p(ws), _p(self.amax), phase,
                                 _p(y) if has_mask else None, _p(dy2), lddy2, _p(keep), _stream()), "bn_bwd")

        call(2, dgamma, dbeta)
        self.pending.append(call)
        self.seen += 1
        if self.seen == self.k:
            self.flush()
        set_amax(dx, self.amax)
        dx._glf_packed_only = True
        dx._glf_grad_group = (self, i)
        return dx

    def flush(self) -> None:
        for call in self.pending:
            call(3)
        self.pending, self.seen = [], 0


class AsppCentreFn(Function):
    """The conv branches of an ASPP head (a 1x1 conv and 3x3 stride-1 pad == dil convs over one input) up to their BatchNorm
    inputs: k outputs, column slices of one [N,H,W,k Cout] buffer, plus the per-branch column statistics [k][2][Cout] (final
    for every branch after the one segmented launch, _aspp_fwd_one; otherwise for the 1x1 branch and for every 3x3 branch
    whose kept taps are the centre alone)."""

    @staticmethod
    def forward(ctx, x, dils, stats: bool, *weights):
        x = _contig(_chk(x, "conv input"))
        n, h, w, cin = x.shape
        k, cout = len(weights), weights[0].shape[0]
        rows, ldu, dev = n * h * w, k * cout, x.device
        am_x = amax_of(x)
        U = torch.empty(n, h, w, ldu, dtype=torch.float32, device=dev)
        sums = stats_slot(ldu, dev) if stats else None
        # one segmented launch stores U and the statistics of every branch; where it does not apply: the stacked centre launch,
        # then one adding launch per branch that keeps off-centre taps
        xa = _aspp_fwd_one(x, am_x, weights, dils, U, sums, n, h, w, cin, cout)
        one, pa = xa is not None, xa is not None
        if not one:
            Wc = aspp_centre_weights(weights)
            am_wc = amax_of(Wc)
            ok = nt_presplit_ok(cin, cin, cin)
            ok_x = ok and (ldu >= PRESPLIT_MIN_COLS or packed_hit(x, am_x) is not None)
            xa, pa = pick(x, act_packed(x, am_x) if ok_x else None, ok_x)
            wb, pb = pick(Wc, weight_packed(Wc, Wc, "w", am_wc) if ok else None, ok)
            gemm("nt", xa, wb, U, M=rows, N=ldu, K=cin, lda=cin, ldb=cin, ldc=ldu, amax_a=am_x, amax_b=am_wc, colstats=sums,
                 a_packed=pa, b_packed=pb)
        for i in range(1, 1 if one else k):
            d = dils[i - 1]
            # the launch this conv would use alone (per-tap rectangles with atomics, or dense), minus the centre tap: it adds into
            # its column slice of U, which needs no zero fill
            pl = conv_plan.plan("fwd", (n, h, w, cin, cout, 3, 3, 1, d, d), _PREC[0], keep=~CENTRE_TAP)
            if not pl.mask:
                continue
            wt, am_w = tap_major(weights[i]), amax_of(weights[i])
            ok_xi = ok and (cout * pl.kept >= PRESPLIT_MIN_COLS or packed_hit(x, am_x) is not None)
            xi, pi = pick(x, act_packed(x, am_x) if ok_xi else None, ok_xi)
            wi, pbi = pick(wt, weight_packed(wt, weights[i], "w", am_w) if ok else None, ok)
            gemm("nt", xi, wi, U[..., i * cout:(i + 1) * cout], M=rows, N=cout, K=cin, lda=cin, ldb=cin, ldc=ldu, taps=9, mask=pl.mask,
                 tap_stride_b=cout * cin, gather=1, geo=pl.geo, rect=pl.rect, accumulate=not pl.rect,
                 amax_a=am_x, amax_b=am_w, a_packed=pi, b_packed=pbi)
        # [2][k Cout] -> [k][2][Cout]: the layout a BatchNorm reads its own sums in (a 16 KB copy)
        s4 = sums.view(2, k, cout).permute(1, 0, 2).contiguous() if stats else torch.empty(0, dtype=torch.float64, device=dev)
        s4._glf_final_all = one                  # the one launch counted every branch's elements: no BatchNorm reduces its own
        ctx.mark_non_differentiable(s4)
        ctx.save_for_backward(x)
        ctx.x_packed = (xa, am_x) if (pa and packed_hit(x, am_x) is not None) else None
        ctx.weights, ctx.dils = weights, dils
        ctx.group = grp = _GradGroup(k, cout)
        outs = tuple(U[..., i * cout:(i + 1) * cout] for i in range(k))
        for i, t in enumerate(outs):
            t._glf_grad_group = (grp, i)
        return outs + (s4,)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        x, = ctx.saved_tensors
        weights, dils, grp = ctx.weights, ctx.dils, ctx.group
        n, h, w, cin = x.shape
        k, cout = len(weights), weights[0].shape[0]
        rows, ldu, dev = n * h * w, k * cout, x.device
        grp.flush()
        G, am_g = grp.G, grp.amax
        for i in range(k):
            if G is None or getattr(dys[i], "_glf_grad_group", None) != (grp, i) or dys[i].data_ptr() != G.data_ptr() + 4 * i * cout:
                raise RuntimeError("glfusion_amd: AsppCentreFn needs every branch's gradient from the BatchNorm that follows it")
        Wc = aspp_centre_weights(weights)
        am_wc = amax_of(Wc)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            slot = amax_slot(dev)
            # one segmented launch stores dx; where it does not apply: the stacked centre launch, then one accumulating launch per
            # branch that keeps off-centre taps
            one = _aspp_dgrad_one(G, am_g, weights, dils, dx, slot, n, h, w, cin, cout)
            if not one:
                WcT = weight_T(Wc, Wc)
                wb, pb = pick(WcT, weight_packed(WcT, Wc, "wT", am_wc), True)
                gemm("nt", G, wb, dx, M=rows, N=cin, K=ldu, lda=ldu, ldb=ldu, ldc=cin, amax_a=am_g, amax_b=am_wc, amax_c=slot,
                     a_packed=True, b_packed=pb)
            for i in range(1, 1 if one else k):
                d = dils[i - 1]
                # (region mode: a region whose taps are all masked out gets no tiles, its pixels are not touched)
                pl = conv_plan.plan("dgrad", (n, h, w, cin, cout, 3, 3, 1, d, d), _PREC[0], keep=~CENTRE_TAP)
                if not pl.mask:
                    continue
                rect = pl.rect
                wT, am_w = tap_major_T(weights[i]), amax_of(weights[i])
                wi, pbi = pick(wT, weight_packed(wT, weights[i], "wT", am_w), True)
                gemm("nt", dys[i], wi, dx, M=rows, N=cin, K=cout, lda=ldu, ldb=cout, ldc=cin, taps=9, mask=pl.mask, tap_stride_b=cout * cin,
                     gather=2, geo=pl.geo, rect=rect, accumulate=rect != 1, amax_a=am_g, amax_b=am_w,
                     amax_c=slot if rect != 1 else None, a_packed=True, b_packed=pbi)
                if rect == 1:
                    slot = None                  # atomics report no maximum: dx is measured on first use
            set_amax(dx, slot)
            dx._glf_owned = True                 # fresh and handed to ONE consumer: a fan_out node may add into it
        dws = []
        # every centre weight wanted: their gradients are ONE plain reduction dWc [k Cout][Cin] = G^T x over the full map (the 1x1
        # weight's is row block 0; row block i is the centre tap of branch i, which the store of that branch's gradient picks up)
        stacked = ASPP_CENTRE_WGRAD and all(ctx.needs_input_grad[3:3 + k])
        if stacked:
            dWc = torch.empty(ldu, cin, dtype=torch.float32, device=dev)
            am_x = ctx.x_packed[1] if ctx.x_packed is not None else amax_of(x)
            xb, pb = pick(x, ctx.x_packed[0] if ctx.x_packed is not None else None, tn_presplit_ok(ldu, cin, ldu, cin))
            gemm("tn", G, xb, dWc, M=ldu, N=cin, K=rows, lda=ldu, ldb=cin, ldc=cin, split=conv_plan.wgrad_split(rows, 1.0, ldu, cin, 1, False, _PREC[0]),
                 amax_a=am_g, amax_b=am_x, a_packed=True, b_packed=pb)
        for i in range(k):
            if not ctx.needs_input_grad[3 + i]:
                dws.append(None)
                continue
            kk, d = (1, 1) if i == 0 else (3, dils[i - 1])
            geom = (n, h, w, cin, cout, kk, kk, 1, 0 if i == 0 else d, d)
            if stacked and i == 0:
                # a copy of 4 Cout Cin bytes (2 MB at 2048 -> 256) into the parameter's slot; the alternative, a reduce that sends
                # one row block elsewhere, would put a second destination into every TN second stage for this one caller
                dw = grad_out(weights[0], tuple(weights[0].shape), dev)
                if dw.data_ptr() % 16 == 0:
                    check(lib.glf_copy_frames(_p(dWc), cout * cin, _p(dw), cout * cin, 1, cout * cin, _stream()), "aspp_centre(dw 1x1)")
                else:                      # (a bucket slot that starts off a 16-byte boundary: the branch's own reduction stores there)
                    _conv_wgrad(weights[0], tuple(weights[0].shape), x, ctx.x_packed, dys[0], ldu, True, am_g,
                                    conv_plan.plan("wgrad", geom, _PREC[0]), out=dw)
                dws.append(dw)
            elif stacked:
                dws.append(_conv_wgrad(weights[i], tuple(weights[i].shape), x, ctx.x_packed, dys[i], ldu, True, am_g,
                                       conv_plan.plan("wgrad", geom, _PREC[0], keep=~CENTRE_TAP), foreign=(4, dWc[i * cout:(i + 1) * cout], cin)))
            else:
                dws.append(_conv_wgrad(weights[i], tuple(weights[i].shape), x, ctx.x_packed, dys[i], ldu, True, am_g,
                                       conv_plan.plan("wgrad", geom, _PREC[0])))
        return (dx, None, None) + tuple(dws)


def aspp_centre_convs(x, convs, stats: bool):
    """The conv outputs of the ASPP conv branches `convs` (see aspp_centre_ok) and, with stats, their column statistics:
    ([u_0 .. u_{k-1}], [sums_i or None]) -- every branch gets its sums from the one segmented launch (ASPP_FWD_ONE); on the
    other route sums_i is None where branch i kept off-centre taps (its BatchNorm reduces its own statistics)."""
    n, h, w = x.shape[0], x.shape[1], x.shape[2]
    dils = tuple(int(cv.dilation[0]) for cv in convs[1:])
    out = AsppCentreFn.apply(x, dils, bool(stats), *[cv.weight for cv in convs])
    us, s4 = out[:-1], out[-1]
    all_final = bool(getattr(s4, "_glf_final_all", False))
    final = [True] + [all_final or (tap_mask(1, h, w, h, w, 3, 3, 1, d, d) & ~CENTRE_TAP) == 0 for d in dils]
    return list(us), [s4[i] if (stats and f) else None for i, f in enumerate(final)]


class ConvCatFn(Function):
    """1x1 conv over the channel-concatenation of several [N,H,W,Ck] inputs WITHOUT materialising
    the concat (ASPP project, deeplabv3.py:153-165): y = sum_k x_k @ W[:, slice_k]^T."""

    @staticmethod
    def forward(ctx, weight, bias, *xs):
        _chk(weight, "weight")
        cout, ctot = weight.shape[0], weight.shape[1]
        w2 = _contig(weight.detach()).view(cout, ctot)
        rows = xs[0].numel() // xs[0].shape[-1]
        # inputs that ARE the column slices of one [..., ctot] buffer (ops.output_into): one K = ctot contraction
        t0 = _chk(xs[0], "input")
        offs = [0]
        for t in xs:
            offs.append(offs[-1] + t.shape[-1])
        ctx.cat = (offs[-1] == ctot and not t0.is_contiguous() and t0.stride(-1) == 1 and t0.stride(-2) == ctot
                   and all(_chk(t, "input").stride() == t0.stride() and t.shape[:-1] == t0.shape[:-1]
                           and t.data_ptr() == t0.data_ptr() + 4 * o for t, o in zip(xs, offs)))
        if ctx.cat:
            y = torch.empty(*t0.shape[:-1], cout, dtype=torch.float32, device=t0.device)
            am_w = amax_of(weight)
            ok = nt_presplit_ok(ctot, ctot, ctot)
            wb, pb = pick(w2, weight_packed(w2, weight, "w", am_w) if ok else None, ok)
            gemm("nt", t0, wb, y, M=rows, N=cout, K=ctot, lda=ctot, ldb=ctot, ldc=cout, bias=bias,
                 amax_a=amax_of(t0), amax_b=am_w, b_packed=pb)
            ctx.save_for_backward(w2, *xs)
            ctx.wshape = tuple(weight.shape)
            ctx.weight_ref = weight
            ctx.has_bias = bias is not None
            return y
        xs = [_contig(_chk(t, "input")) for t in xs]
        y = torch.empty(*xs[0].shape[:-1], cout, dtype=torch.float32, device=xs[0].device)
        off = 0
        for i, t in enumerate(xs):
            ck = t.shape[-1]
            gemm("nt", t, w2[:, off:], y, M=rows, N=cout, K=ck, lda=ck, ldb=ctot, ldc=cout, accumulate=i > 0,
                 bias=bias if i == 0 else None, amax_a=amax_of(t), amax_b=amax_of(weight))
            off += ck
        if off != ctot:
            raise RuntimeError(f"conv_cat: inputs have {off} channels in total, weight expects {ctot}")
        ctx.save_for_backward(w2, *xs)
        ctx.wshape = tuple(weight.shape)
        ctx.weight_ref = weight
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        w2, *xs = ctx.saved_tensors
        dy = _contig(dy)
        cout, ctot = w2.shape
        rows = dy.numel() // cout
        split = _tn_split(rows, cout, xs[0].shape[-1], 1)
        dw = None
        if ctx.needs_input_grad[0]:
            dw = torch.empty(cout, ctot, dtype=torch.float32, device=dy.device)
        db = colsum(dy, rows, cout) if (ctx.has_bias and ctx.needs_input_grad[1]) else None
        grads = []
        off = 0
        am_dy, am_w = amax_of(dy), amax_of(ctx.weight_ref)
        dy_pk = packed_only(dy)
        if dy_pk and (not ctx.cat or ctx.has_bias or am_dy is None or not (split_mode() and cout % 32 == 0)):
            raise RuntimeError("glfusion_amd: a packed-only gradient reached a projection that cannot consume it")
        if ctx.cat:
            t0 = xs[0]
            if any(ctx.needs_input_grad[2:]):
                dcat = torch.empty(*t0.shape[:-1], ctot, dtype=torch.float32, device=dy.device)
                am_dc = amax_slot(dy.device)
                if split_mode() and cout % 32 == 0:
                    w2T = weight_T(w2, ctx.weight_ref)
                    ok = nt_presplit_ok(cout, cout, cout)
                    da, pa = (dy, True) if dy_pk else pick(dy, act_packed(dy, am_dy, True) if ok else None, ok)
                    wb, pb = pick(w2T, weight_packed(w2T, ctx.weight_ref, "T2", am_w) if ok else None, ok)
                    gemm("nt", da, wb, dcat, M=rows, N=ctot, K=cout, lda=cout, ldb=cout, ldc=ctot,
                         amax_a=am_dy, amax_b=am_w, amax_c=am_dc, a_packed=pa, b_packed=pb)
                else:
                    am_dc = None
                    gemm("nn", dy, w2, dcat, M=rows, N=ctot, K=cout, lda=cout, ldb=ctot, ldc=ctot)
                for t in xs:
                    g = dcat[..., off:off + t.shape[-1]]
                    set_amax(g, am_dc)
                    grads.append(g)
                    off += t.shape[-1]
            else:
                grads = [None] * len(xs)
            if dw is not None:
                split = _tn_split(rows, cout, ctot, 1)
                ok = tn_presplit_ok(cout, ctot, cout, ctot)
                da, pa = (dy, True) if dy_pk else pick(dy, act_packed(dy, am_dy, True) if ok else None, ok)
                gemm("tn", da, t0, dw, M=cout, N=ctot, K=rows, lda=cout, ldb=ctot, ldc=ctot, split=split,
                     amax_a=am_dy, amax_b=amax_of(t0), a_packed=pa)
            return (dw.view(ctx.wshape) if dw is not None else None, db, *grads)
        for i, t in enumerate(xs):
            ck = t.shape[-1]
            if ctx.needs_input_grad[2 + i]:
                dx = torch.empty_like(t)
                if split_mode() and cout % 32 == 0:
                    wT = weight_T(w2, ctx.weight_ref)                     # [ctot][cout]
                    gemm("nt", dy, wT[off:], dx, M=rows, N=ck, K=cout, lda=cout, ldb=cout, ldc=ck, amax_a=am_dy, amax_b=am_w)
                else:
                    gemm("nn", dy, w2[:, off:], dx, M=rows, N=ck, K=cout, lda=cout, ldb=ctot, ldc=ck)
                grads.append(dx)
            else:
                grads.append(None)
            if dw is not None:
                gemm("tn", dy, t, dw[:, off:], M=cout, N=ck, K=rows, lda=cout, ldb=ck, ldc=ctot, split=split,
                     amax_a=am_dy, amax_b=amax_of(t))
            off += ck
        return (dw.view(ctx.wshape) if dw is not None else None, db, *grads)


def conv1x1_cat(weight, xs: Sequence[torch.Tensor], bias=None, colstats=None):
    if _is16(xs[0]):
        from . import ops16
        return ops16.conv1x1_cat(weight, xs, bias, colstats)
    if colstats is not None:
        raise RuntimeError("glfusion_amd: conv1x1_cat honours colstats in 16-bit storage mode only")
    return ConvCatFn.apply(weight, bias, *xs)


# ----------------------------------------------------------------------------------------
# stem: Conv2d(1, 64, 7, stride 1, pad p) + bias   (models/_utils.py:192)
# ----------------------------------------------------------------------------------------
class StemFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, pad: int):
        _chk(x, "stem input"); _chk(weight, "stem weight")
        x = _contig(x)                                  # [N,H,W,1]
        n, h, w, _ = x.shape
        cout = weight.shape[0]
        y = torch.empty(n, h + 2 * pad - 6, w + 2 * pad - 6, cout, dtype=torch.float32, device=x.device)
        check(lib.glf_stem7x7_fwd(_p(x), _p(_contig(weight.detach())), _p(bias), _p(y), n, h, w, cout, pad, _stream()), "stem7x7_fwd")
        ctx.save_for_backward(x, weight)
        ctx.cfg = (n, h, w, cout, pad, tuple(weight.shape), bias is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        n, h, w, cout, pad, wshape, has_bias = ctx.cfg
        dy = _contig(dy)
        dx = None
        if ctx.needs_input_grad[0]:                     # the image is itself computed: early_fusion's learned mix of the views
            dx = torch.empty_like(x)
            check(lib.glf_stem7x7_dgrad(_p(dy), _p(_contig(weight.detach())), _p(dx), n, h, w, cout, pad, _stream()), "stem7x7_dgrad")
        dw = torch.empty(wshape, dtype=torch.float32, device=dy.device)
        db = torch.empty(cout, dtype=torch.float32, device=dy.device) if has_bias else None
        part = torch.empty(int(lib.glf_stem7x7_wgrad_workspace(n, h, w, cout, pad)), dtype=torch.float32, device=dy.device)
        check(lib.glf_stem7x7_wgrad(_p(x), _p(dy), _p(dw), _p(db), _p(part), n, h, w, cout, pad, _stream()), "stem7x7_wgrad")
        return dx, dw, db, None


def stem7x7(x, weight, bias, pad: int):
    if _S16[0]:                          # fp32 image in, bf16 conv output: the entry into the 16-bit domain
        from . import ops16
        return ops16.stem7x7(x, weight, bias, pad)
    return StemFn.apply(x, weight, bias, pad)


FUSED_STEM = os.environ.get("GLF_FUSED_STEM", "1") != "0"


def stem_bn_relu_pool(x, weight, bias, running_mean, running_var, gamma, beta, eps: float, pad: int):
    """Inference-mode init_block in one launch (glf_stem7x7_bn_relu_pool): maxpool3x3s2(relu(bn_eval(conv7x7(x) + bias))) on
    [N,H,W,1] -> [N,Hp,Wp,64].  Forward only (no autograd node): for no_grad evaluation."""
    _chk(x, "stem input"); _chk(weight, "stem weight")
    x = _contig(x)
    n, h, w, _ = x.shape
    cout = weight.shape[0]
    ho, wo = h + 2 * pad - 6, w + 2 * pad - 6
    dev = x.device
    mean = torch.empty(cout, dtype=torch.float32, device=dev)
    invstd = torch.empty(cout, dtype=torch.float32, device=dev)
    check(lib.glf_bn_eval_coeffs(_p(running_mean), _p(running_var), eps, _p(mean), _p(invstd), cout, _stream()), "bn_eval_coeffs")
    y = torch.empty(n, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1, cout, dtype=torch.float32, device=dev)
    am = amax_slot(dev)
    check(lib.glf_stem7x7_bn_relu_pool(_p(x), _p(_contig(weight.detach())), _p(bias), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(y),
                                       n, h, w, cout, pad, _p(am), _stream()), "stem7x7_bn_relu_pool")
    set_amax(y, am)
    return y


# ----------------------------------------------------------------------------------------
# writing a branch's last kernel straight into a column slice of a wider buffer (ASPP: no concat, ONE projection GEMM)
# ----------------------------------------------------------------------------------------
_OUT_VIEW = [None]


class output_into:
    """Within the block, the next BatchNorm-apply / broadcast whose output has `view`'s shape writes into `view` (a
    [..., C] column slice of a wider channels-last buffer: row stride = the buffer's channel count) instead of a
    fresh tensor, and reports its maximum into `amax` (a slot shared by all writers of the buffer)."""

    def __init__(self, view: torch.Tensor, amax: Optional[torch.Tensor] = None):
        self.item = (view, amax)

    def __enter__(self):
        _OUT_VIEW[0] = self.item
        return self

    def __exit__(self, *exc):
        _OUT_VIEW[0] = None
        return False


def _take_out(shape, device, dtype=torch.float32):
    """(output tensor, row stride, shared amax slot or None) for a [..., C] result of `shape`: the pending output_into view when
    it matches, a fresh tensor otherwise.  Only fp32 storage carries maxima."""
    item = _OUT_VIEW[0]
    if item is not None and tuple(item[0].shape) == tuple(shape) and item[0].stride(-1) == 1 and item[0].dtype == dtype:
        _OUT_VIEW[0] = None
        return item[0], int(item[0].stride(-2)), item[1] if dtype == torch.float32 else None
    return torch.empty(tuple(shape), dtype=dtype, device=device), int(shape[-1]), None


def _rows_view(t: torch.Tensor):
    """(tensor, row stride) for reading a [..., C] tensor as rows: contiguous, or a column slice of a wider
    channels-last buffer (uniform row stride; bf16: one the 16-byte accesses can walk); anything else is copied."""
    if t.is_contiguous():
        return t, int(t.shape[-1])
    if t.dim() >= 2 and t.stride(-1) == 1:
        ld = int(t.stride(-2))
        ok = all(t.stride(d) == t.stride(d + 1) * t.shape[d + 1] for d in range(t.dim() - 2))
        if ok and ld >= t.shape[-1] and (not _is16(t) or (ld % 8 == 0 and t.data_ptr() % 16 == 0)):
            return t, ld
    t = t.contiguous()
    return t, int(t.shape[-1])


# ----------------------------------------------------------------------------------------
# BatchNorm (+ residual, + ReLU)
# ----------------------------------------------------------------------------------------
_last_bn = [None]          # (mean, invstd, rows) of the most recent BatchNormActFn.forward (read by BN_TAP)


class BatchNormActFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, nbt, training: bool,
                momentum: float, eps: float, relu: bool, sums=None, packed_grad: bool = False, packed_out: bool = False):
        _chk(x, "bn input"); _chk(gamma, "bn weight"); _chk(beta, "bn bias")
        ctx.grad_group = getattr(x, "_glf_grad_group", None)      # AsppCentreFn: dx goes into a column slice of a shared packed image
        x, ldx = _rows_view(x)                   # may be a column slice of the stacked centre-tap conv output
        c = x.shape[-1]
        rows = x.numel() // c
        dev = x.device
        mean = torch.empty(c, dtype=torch.float32, device=dev)
        invstd = torch.empty(c, dtype=torch.float32, device=dev)
        fused_stats = training and sums is not None and c <= 4096
        if fused_stats:
            pass                                 # finished inside the apply kernel below (one launch)
        elif training and sums is not None:      # (sum x, sum x^2) came out of the producing contraction's epilogue
            check(lib.glf_bn_stats_from_sums(_p(sums), rows, c, eps, momentum, _p(mean), _p(invstd), _p(running_mean),
                                             _p(running_var), _p(nbt), _stream()), "bn_stats_from_sums")
        elif training:
            check(lib.glf_bn_stats(_p(x), ldx, rows, c, eps, momentum, _p(mean), _p(invstd), _p(running_mean), _p(running_var),
                                   _p(nbt), _p(_ws(rows, c, dev)), _stream()), "bn_stats")
        else:
            if running_mean is None or running_var is None:
                raise RuntimeError("batch_norm in eval mode needs running statistics")
            check(lib.glf_bn_eval_coeffs(_p(running_mean), _p(running_var), eps, _p(mean), _p(invstd), c, _stream()), "bn_eval_coeffs")
        if residual is not None:
            residual = _contig(_chk(residual, "bn residual"))
        # packed_out: the only reader is a convolution that takes its input as a packed pre-split image -- write that, once,
        # scaled by a bound of max |y| derived from the conv epilogue's per-channel maxima (no fp32 y, no split pass)
        colmax = getattr(sums, "_glf_colmax", None) if sums is not None else None
        packed = (bool(packed_out) and fused_stats and residual is None and colmax is not None and _PREC[0] >= 2
                  and PACKED_ACTS and _OUT_VIEW[0] is None)
        y, ldy, shared = _take_out(x.shape, dev)
        am = shared if shared is not None else amax_slot(dev)
        packed = packed and am is not None
        # relu + residual: the backward needs the sign of the forward output -- kept as one byte per four channels instead of y
        # (grad mode is always OFF inside Function.forward: before round 4 this read torch.is_grad_enabled() and the sign bytes were
        # never produced -- the backward fell back to re-reading y; what says that a backward may follow is needs_input_grad)
        need_mask = relu and residual is not None and any(ctx.needs_input_grad[:4])
        mask = torch.empty(rows * (c // 4), dtype=torch.uint8, device=dev) if need_mask else None
        if fused_stats:
            check(lib.glf_bn_apply_from_sums(_p(x), ldx, _p(residual), c, _p(y), ldy, _p(sums), rows, c, eps, momentum, _p(gamma), _p(beta),
                                             _p(mean), _p(invstd), _p(running_mean), _p(running_var), _p(nbt), int(relu), _p(am),
                                             _p(mask), _p(colmax) if packed else None, _stream()), "bn_apply_from_sums")
        else:
            check(lib.glf_bn_apply(_p(x), ldx, _p(residual), c, _p(y), ldy, _p(mean), _p(invstd), _p(gamma), _p(beta), rows, c,
                                   int(relu), _p(am), _p(mask), _stream()), "bn_apply")
        set_amax(y, am)
        if packed:
            y._glf_packed_only = True
        # without a residual the ReLU mask is recomputed from x in backward (sign of the same expression): y is not kept
        ctx.save_for_backward(x, mask if need_mask else (y if (relu and residual is not None) else None), mean, invstd, gamma, beta if relu else None)
        ctx.has_mask = need_mask
        ctx.cfg = (rows, c, relu, training, residual is not None, ldy, ldx)
        ctx.packed_grad = bool(packed_grad) and _PREC[0] >= 2
        ctx.param_refs = (gamma, beta)
        _last_bn[0] = (mean, invstd, rows)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, y, mean, invstd, gamma, beta = ctx.saved_tensors
        rows, c, relu, training, has_res, ldy, ldx = ctx.cfg
        dy2 = getattr(dy, "_glf_addend", None)    # fan_out(lazy=True): the two gradients of a block input arrive unsummed
        lddy2 = 0
        dy, lddy = _rows_view(dy)                 # may be a column slice of the concat-free projection's gradient
        if dy2 is not None:
            if dy2.shape != dy.shape:
                raise RuntimeError("glfusion_amd: the two addends of a lazy fan-in gradient differ in shape")
            dy2, lddy2 = _rows_view(dy2)
        dev = dy.device
        dres = torch.empty(x.shape, dtype=torch.float32, device=dev) if (has_res and ctx.needs_input_grad[3]) else None
        dgamma = grad_out(ctx.param_refs[0], (c,), dev)
        dbeta = grad_out(ctx.param_refs[1], (c,), dev)
        if ctx.grad_group is not None:
            return (ctx.grad_group[0].bn_backward(ctx.grad_group[1], dy, lddy, dy2, lddy2, x, ldx, y, ldy, mean, invstd, gamma, beta, dgamma, dbeta,
                                                  rows, c, relu, training, ctx.has_mask), dgamma, dbeta) + (None,) * 11
        dx = torch.empty(x.shape, dtype=torch.float32, device=dev)
        am = amax_slot(dev)
        # packed: the producing conv reads this gradient only through its dgrad / wgrad contractions -- write it ONCE, as the
        # packed pre-split image they want (scaled by a bound of its maximum the reduction pass provides), instead of fp32
        # followed by a split pass
        packed = ctx.packed_grad and _PREC[0] >= 2 and am is not None and PACKED_GRADS
        mask = y if ctx.has_mask else None
        fused = bnbwd_slot(c, dev) if c <= 4096 else None      # two launches (atomics) instead of three
        check(lib.glf_bn_bwd(_p(dy), lddy, _p(x), ldx, None if ctx.has_mask else _p(y), ldy, _p(mean), _p(invstd), _p(gamma), _p(beta),
                             _p(dx), c, _p(dres), c, _p(dgamma), _p(dbeta), rows, c, int(relu), int(training),
                             None if fused is not None else _p(_ws(rows, c, dev)), _p(am), int(packed), _p(mask), _p(dy2), lddy2, _p(fused), _stream()), "bn_bwd")
        set_amax(dx, am)
        if packed:
            dx._glf_packed_only = True
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None, None, None, None


# When a list, every train-mode batch_norm_act call appends (module, batch mean, batch invstd, rows): enough to
# replay the running-statistics update of a layer whose output is being reused instead of recomputed.
BN_TAP = None


def replay_bn_updates(records) -> None:
    """Apply again the running-stat updates recorded by BN_TAP (same batch statistics): what a second forward of the
    same modules over the same input would have done to running_mean / running_var / num_batches_tracked."""
    for bn, mean, invstd, rows in records:
        if not bn.track_running_stats or bn.running_mean is None:
            continue
        stats_moved(bn)
        check(lib.glf_bn_replay_running(_p(mean), _p(invstd), int(rows), mean.numel(), float(bn.eps), float(bn.momentum),
                                        _p(bn.running_mean), _p(bn.running_var), _p(bn.num_batches_tracked), _stream()), "bn_replay_running")


# BatchNorm backward hands the gradient of a conv output to that conv as a packed pre-split image (no fp32 copy, no split pass)
PACKED_GRADS = os.environ.get("GLF_PACKED_GRADS", "1") != "0"


def takes_packed_grad(weight: torch.Tensor) -> bool:
    """True when Conv2dFn / ConvCatFn backward can consume the gradient of a conv's output as a packed-only image: both its
    dgrad (NT, K = Cout) and its weight gradient (TN, M = Cout, N = Cin) run on the aligned split-fp16 kernels."""
    if not PACKED_GRADS or _PREC[0] < 2 or not PRESPLIT:
        return False
    cout, cin = weight.shape[0], weight.shape[1]
    return cout % 32 == 0 and nt_presplit_ok(cout, cout, cout) and tn_presplit_ok(cout, cin, cout, cin)


# BatchNorm forward hands an activation whose only reader is a convolution to it as a packed pre-split image
PACKED_ACTS = os.environ.get("GLF_PACKED_ACTS", "1") != "0"


def takes_packed_input(weight: torch.Tensor) -> bool:
    """True when Conv2dFn can consume its INPUT as a packed-only image: its forward (NT, K = Cin) and its weight gradient
    (TN, N = Cin) both run on the aligned split-fp16 kernels."""
    if not PACKED_ACTS or _PREC[0] < 2 or not PRESPLIT:
        return False
    cout, cin = weight.shape[0], weight.shape[1]
    return cin % 32 == 0 and nt_presplit_ok(cin, cin, cin) and tn_presplit_ok(cout, cin, cout, cin)


def packed_only(t: torch.Tensor) -> bool:
    return bool(getattr(t, "_glf_packed_only", False))


def batch_norm_act(x, bn: torch.nn.modules.batchnorm._BatchNorm, relu: bool, residual=None, sums=None, packed_grad: bool = False,
                   packed_out: bool = False):
    """nn.BatchNorm{2,3}d semantics (train: batch stats + running update; eval: running stats),
    optionally fused with a residual add and ReLU."""
    training = bn.training or bn.running_mean is None
    if training and x.numel() // x.shape[-1] <= 1:
        # same refusal (and wording) as torch.nn.functional.batch_norm in train mode
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {list(from_nhwc(x).shape) if x.dim() == 4 else list(x.shape)}")
    momentum = 0.0 if bn.momentum is None else float(bn.momentum)
    if bn.momentum is None and training and bn.track_running_stats:
        raise RuntimeError("glfusion_amd: cumulative-average BatchNorm (momentum=None) is not built")
    track = training and bn.track_running_stats
    if track:
        stats_moved(bn)                   # the kernels write the running statistics in place: tell the folded images
    if _is16(x):
        from . import ops16
        y = ops16.BatchNormAct16Fn.apply(x, bn.weight, bn.bias, residual,
                                         bn.running_mean if (track or not training) else None,
                                         bn.running_var if (track or not training) else None,
                                         bn.num_batches_tracked if track else None,
                                         training, momentum, float(bn.eps), relu, sums if training else None)
        if BN_TAP is not None and track:
            BN_TAP.append((bn,) + _last_bn[0])
        return y
    y = BatchNormActFn.apply(x, bn.weight, bn.bias, residual,
                             bn.running_mean if (track or not training) else None,
                             bn.running_var if (track or not training) else None,
                             bn.num_batches_tracked if track else None,
                             training, momentum, float(bn.eps), relu, sums if training else None, packed_grad, packed_out)
    if BN_TAP is not None and track:
        BN_TAP.append((bn,) + _last_bn[0])
    return y


# ----------------------------------------------------------------------------------------
# Folded-BatchNorm inference (opt-in: set_fold_bn).  With frozen statistics BatchNorm is an affine map per output channel,
#     W'[o] = W[o] * s_o,   shift_o = beta_o + (bias_o - mean_o) * s_o,   s_o = gamma_o / sqrt(var_o + eps)
# so conv -> BatchNorm (-> + residual) (-> ReLU) is ONE contraction whose epilogue adds the shift and the residual and clamps
# (glf_gemm_nt_epilogue): the conv output is written once instead of written, re-read, and written again.
# ----------------------------------------------------------------------------------------
_FOLD_BN = [False]
_FOLD_BN_S16 = [False]
FOLD_COUNT = [0]            # glf_fold_bn / glf_s16_fold_bn launches so far (a folded image is rebuilt only when one of its six sources changed)
_STATS_GEN = [0]            # bumped when running statistics moved behind Python's back (a replayed training graph)
_fold_cache = {}


def set_fold_bn(flag: bool) -> None:
    """Route eval-mode, no-grad conv -> BatchNorm groups under 'f16x3' / 'f16' through the folded one-launch path.  Off by default;
    every other call (training, recorded graphs, the other precisions, convs the epilogue kernels do not cover) is untouched."""
    _FOLD_BN[0] = bool(flag)


def fold_bn() -> bool:
    return _FOLD_BN[0]


def set_fold_bn_s16(flag: bool) -> None:
    """The same switch for 16-bit storage: eval-mode, no-grad conv -> BatchNorm groups under 'bf16' go through
    ops16.conv_bn_folded16 (one launch, the value rounded to bf16 once, after normalisation).  Off by default and independent of
    set_fold_bn: each switch acts under its own precisions only."""
    _FOLD_BN_S16[0] = bool(flag)


def fold_bn_s16() -> bool:
    return _FOLD_BN_S16[0]


def stats_moved(bn=None) -> None:
    """Running statistics were written by a kernel (torch's version counter does not see raw writes): of `bn`, or -- None -- of
    modules unknown to the caller (engine.StepGraph.replay)."""
    if bn is None:
        _STATS_GEN[0] += 1
        return
    for t in (bn.running_mean, bn.running_var):
        if t is not None:
            t._glf_moved = getattr(t, "_glf_moved", 0) + 1


def _src_stamp(t):
    return None if t is None else (t._version, t.data_ptr(), getattr(t, "_glf_moved", 0))


class _Folded:
    __slots__ = ("wref", "bref", "wf", "shift", "stamp", "gen")


def fold_plan(x: torch.Tensor, weight: torch.Tensor, bn, stride: int, pad: int, dil: int):
    """The conv's "fwd_folded" ConvPlan when conv(x, weight) -> bn runs on the folded path right now, else None: switch on, split-fp16
    precision, no autograd graph, BatchNorm in eval mode with running statistics, and a conv the epilogue kernels cover (aligned
    fast path, more than 64 output rows, every output element stored once: dense, or region mode where the unfolded conv would
    sum per-tap rectangles with atomics and the conv is a 3x3 'same' one; other per-tap-rectangle convs stay unfolded)."""
    if not _FOLD_BN[0] or _PREC[0] < 2 or _S16[0] or torch.is_grad_enabled():
        return None
    if bn.training or bn.running_mean is None or bn.running_var is None or bn.weight is None or bn.bias is None:
        return None
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda or packed_only(x):
        return None
    n, h, w, cin = x.shape
    cout, cin_w, kh, kw = weight.shape
    if cin_w != cin or cin % 32 != 0 or cin > (1 << 18) or cout % 4 != 0:
        return None
    pl = conv_plan.plan("fwd_folded", (n, h, w, cin, cout, kh, kw, stride, pad, dil), _PREC[0])
    # <= 64 rows: the skinny kernel of the ASPP pooled branch keeps its path; rect 1: per-tap rectangles no region mode replaces
    if pl.ho <= 0 or pl.wo <= 0 or pl.M <= 64 or pl.mask == 0 or pl.rect == 1:
        return None
    return pl


def _fold_entry(cache: dict, weight: torch.Tensor, bias: Optional[torch.Tensor], bn, dtype):
    """(cache entry, current stamp) of a conv -> BatchNorm pair in `cache` (one cache per storage type of the folded weights: the
    fp32 images here, the bf16 ones of ops16).  The entry owns the folded weight [taps][Cout][Cin] of `dtype` and the fp32 shift;
    whoever finds entry.stamp != stamp re-folds in place and stores the stamp.  The stamp covers the six sources (version counter,
    data pointer, raw-write note), the global note of statistics moved behind Python's back, and eps."""
    key = (id(weight), id(bn))
    hit = cache.get(key)
    cout, cin, kh, kw = weight.shape
    if hit is None or hit.wref() is not weight or hit.bref() is not bn or hit.wf.device != weight.device or tuple(hit.wf.shape) != (kh * kw, cout, cin):
        hit = _Folded()
        hit.wref = weakref.ref(weight, lambda _r, k=key: cache.pop(k, None))
        hit.bref = weakref.ref(bn)
        hit.wf = torch.empty(kh * kw, cout, cin, dtype=dtype, device=weight.device)
        hit.shift = torch.empty(cout, dtype=torch.float32, device=weight.device)
        hit.stamp, hit.gen = None, 0
        href = weakref.ref(hit.wf)
        hit.wf._glf_version_fn = lambda c=cache, k=key, r=href: (c[k].gen if (k in c and c[k].wf is r()) else -1)
        cache[key] = hit
    stamp = tuple(_src_stamp(t) for t in (weight, bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)) + (_STATS_GEN[0], float(bn.eps))
    return hit, stamp


def _folded_images(weight: torch.Tensor, bias: Optional[torch.Tensor], bn):
    """(folded tap-major weights [taps][Cout][Cin], shift [Cout]) of a conv -> BatchNorm pair: derived images of SIX sources
    (conv weight and bias, gamma, beta, running_mean, running_var), rebuilt in place by one glf_fold_bn launch when the stamp
    (version counter, data pointer, raw-write note) of any of them changed and never otherwise.  The folded weight carries its
    own generation as `_glf_version_fn`, so its maximum and packed pre-split image (registered weight images) follow it."""
    cout, cin, kh, kw = weight.shape
    hit, stamp = _fold_entry(_fold_cache, weight, bias, bn, torch.float32)
    if hit.stamp != stamp:
        wt = tap_major(weight)
        check(lib.glf_fold_bn(_p(wt), _p(bias.detach()) if bias is not None else None, _p(bn.weight.detach()), _p(bn.bias.detach()),
                              _p(bn.running_mean), _p(bn.running_var), float(bn.eps), _p(hit.wf), _p(hit.shift), kh * kw, cout, cin,
                              _stream()), "fold_bn")
        FOLD_COUNT[0] += 1
        hit.gen += 1
        hit.stamp = stamp
    return hit.wf, hit.shift


def conv_bn_folded(x, weight, bias, bn, stride: int, pad: int, dil: int, relu: bool, residual=None, plan=None, amax_x=None):
    """relu?(bn_eval(conv(x)) + residual?) in one launch on NHWC tensors; plan = fold_plan(...) (not None).  amax_x: the bound of
    max|x| when x itself does not carry one (the ASPP concat buffer)."""
    x = _contig(_chk(x, "conv input"))
    n, cin, cout = x.shape[0], x.shape[-1], weight.shape[0]
    wf, shift = _folded_images(weight, bias, bn)
    y, ldy, shared = _take_out((n, plan.ho, plan.wo, cout), x.device)
    am = shared if shared is not None else amax_slot(x.device)
    am_w, am_x = amax_of(wf), (amax_x if amax_x is not None else amax_of(x))
    ok = nt_presplit_ok(cin, cin, cin)
    ok_x = ok and (cout * plan.kept >= PRESPLIT_MIN_COLS or packed_hit(x, am_x) is not None)
    xa, pa = pick(x, act_packed(x, am_x) if ok_x else None, ok_x)
    wb, pb = pick(wf, weight_packed(wf, wf, "w", am_w) if ok else None, ok)
    res, ldr = (None, 0)
    if residual is not None:
        res, ldr = _rows_view(_chk(residual, "bn residual"))
        if res.numel() // res.shape[-1] != plan.M or res.shape[-1] != cout:
            raise RuntimeError("conv_bn_folded: residual shape does not match the conv output")
    gemm("nt", xa, wb, y, M=plan.M, N=cout, K=cin, lda=cin, ldb=cin, ldc=ldy, bias=shift, taps=plan.taps, mask=plan.mask,
         tap_stride_b=cout * cin, gather=plan.gather, geo=plan.geo, rect=plan.rect,
         amax_a=am_x, amax_b=am_w, amax_c=am, a_packed=pa, b_packed=pb, epilogue=(res, ldr, relu))
    set_amax(y, am)
    return y


# ----------------------------------------------------------------------------------------
# ReLU / dropout / pooling
# ----------------------------------------------------------------------------------------
class ReluFn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _contig(_chk(x, "relu input", None))
        y = torch.empty_like(x)
        _launch("relu_fwd", x, x, y, x.numel())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _contig(dy)
        dx = torch.empty_like(dy)
        _launch("relu_bwd", dy, dy, y, dx, dy.numel())
        return dx


def relu(x):
    return ReluFn.apply(x)


class DropoutFn(Function):
    @staticmethod
    def forward(ctx, x, p: float, seed: int):
        x = _contig(_chk(x, "dropout input", None))
        y = torch.empty_like(x)
        _launch("dropout", x, x, y, x.numel(), p, seed, step_counter(x.device))
        amax_bound(y, [x], scale=1.0 / (1.0 - p))          # kept elements are scaled by 1 / (1 - p)
        ctx.cfg = (p, seed)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        p, seed = ctx.cfg
        dy = _contig(dy)
        dx = torch.empty_like(dy)
        _launch("dropout", dy, dy, dx, dy.numel(), p, seed, step_counter(dy.device))
        return dx, None, None


def dropout(x, p: float, training: bool):
    if not training or p <= 0.0:
        return x
    if p >= 1.0:
        raise RuntimeError("dropout p must be < 1")
    seed = int(torch.empty((), dtype=torch.int64).random_(0, 2 ** 62).item())   # host RNG: no device sync
    return DropoutFn.apply(x, float(p), seed)


class MaxPool3x3s2Fn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _contig(_chk(x, "maxpool input", None))
        n, h, w, c = x.shape
        ho, wo = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        y = torch.empty(n, ho, wo, c, dtype=x.dtype, device=x.device)
        idx = torch.empty(n, ho, wo, c, dtype=torch.uint8, device=x.device)
        _launch("maxpool3x3s2_fwd", x, x, y, idx, n, h, w, c)
        amax_bound(y, [x])                                  # a window maximum never exceeds the input's largest magnitude
        ctx.save_for_backward(idx)
        ctx.cfg = (n, h, w, c)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        n, h, w, c = ctx.cfg
        dy = _contig(dy)
        dx = torch.empty(n, h, w, c, dtype=dy.dtype, device=dy.device)
        _launch("maxpool3x3s2_bwd", dy, dy, idx, dx, n, h, w, c)
        return dx


def maxpool3x3s2(x):
    return MaxPool3x3s2Fn.apply(x)


# ----------------------------------------------------------------------------------------
# the streaming pieces of the U-Net baselines (ours.py:2385-2625; csrc/unet_ops.hip)
# ----------------------------------------------------------------------------------------
def _dense_act(x, name: str):
    """A streaming node reads its input as values: a packed-only activation (a BatchNorm output written for ONE convolution) has none."""
    if packed_only(x):
        raise RuntimeError(f"glfusion_amd: a packed-only activation reached {name}, which cannot consume it")
    return _contig(_chk(x, name + " input", None))


class Conv3x3C1Fn(Function):
    """Conv2d(1, 64, 3, stride 1, padding 1) + bias on an fp32 [N,H,W,1] image; the result is fp32, or bf16 under 16-bit storage
    (the entry into the 16-bit domain, as for the stem)."""

    @staticmethod
    def forward(ctx, x, weight, bias, out16: bool):
        _chk(x, "conv3x3_c1 input"); _chk(weight, "conv3x3_c1 weight")
        x = _contig(x)                                  # [N,H,W,1]
        n, h, w, _ = x.shape
        cout = weight.shape[0]
        y = torch.empty(n, h, w, cout, dtype=BF if out16 else torch.float32, device=x.device)
        _launch("conv3x3_c1_fwd", y, x, _contig(weight.detach()), bias, y, n, h, w, cout)
        ctx.save_for_backward(x)
        ctx.cfg = (n, h, w, cout, tuple(weight.shape), bias is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        n, h, w, cout, wshape, has_bias = ctx.cfg
        if ctx.needs_input_grad[0]:
            raise RuntimeError("glfusion_amd: gradient w.r.t. the input image is not on the path (stem dgrad not built)")
        dy = _contig(dy)
        dw = torch.empty(wshape, dtype=torch.float32, device=dy.device)
        db = torch.empty(cout, dtype=torch.float32, device=dy.device) if has_bias else None
        part = torch.empty(int(lib.glf_conv3x3_c1_wgrad_workspace(n, h, w, cout)), dtype=torch.float32, device=dy.device)
        _launch("conv3x3_c1_wgrad", dy, x, dy, dw, db, part, part.numel(), n, h, w, cout)
        return None, dw, db, None


def conv3x3_c1(x, weight, bias):
    return Conv3x3C1Fn.apply(x, weight, bias, _S16[0])


class MaxPool2x2s2Fn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _dense_act(x, "maxpool2x2s2")
        n, h, w, c = x.shape
        y = torch.empty(n, h // 2, w // 2, c, dtype=x.dtype, device=x.device)
        idx = torch.empty(n, h // 2, w // 2, c, dtype=torch.uint8, device=x.device)
        _launch("maxpool2x2s2_fwd", x, x, y, idx, n, h, w, c)
        amax_bound(y, [x])                                  # a window maximum never exceeds the input's largest magnitude
        ctx.save_for_backward(idx)
        ctx.cfg = (n, h, w, c)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        n, h, w, c = ctx.cfg
        dy = _contig(dy)
        dx = torch.empty(n, h, w, c, dtype=dy.dtype, device=dy.device)      # the kernel writes every element, zeros included
        _launch("maxpool2x2s2_bwd", dy, dy, idx, dx, n, h, w, c)
        return dx


def maxpool2x2s2(x):
    return MaxPool2x2s2Fn.apply(x)


class Upsample2xFn(Function):
    """nn.Upsample(scale_factor=2), nearest."""

    @staticmethod
    def forward(ctx, x):
        x = _dense_act(x, "upsample2x")
        n, h, w, c = x.shape
        y = torch.empty(n, 2 * h, 2 * w, c, dtype=x.dtype, device=x.device)
        _launch("upsample2x_fwd", x, x, y, n, h, w, c)
        amax_bound(y, [x])                                  # the same values, four times
        ctx.cfg = (n, h, w, c)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        n, h, w, c = ctx.cfg
        dy = _contig(dy)
        dx = torch.empty(n, h, w, c, dtype=dy.dtype, device=dy.device)
        _launch("upsample2x_bwd", dy, dy, dx, n, h, w, c)
        return dx


def upsample2x(x):
    return Upsample2xFn.apply(x)


class ConcatChannelsFn(Function):
    """torch.cat((a, b), dim=1) on channels-last tensors [..., Ca], [..., Cb] -> [..., Ca + Cb]; a source may be a column slice of a
    wider channels-last buffer."""

    @staticmethod
    def forward(ctx, a, b):
        for t in (a, b):
            if packed_only(t):
                raise RuntimeError("glfusion_amd: a packed-only activation reached concat_channels, which cannot consume it")
        _chk(a, "concat input", None); _chk(b, "concat input", a.dtype)
        if a.shape[:-1] != b.shape[:-1]:
            raise RuntimeError(f"concat_channels: leading extents differ ({tuple(a.shape)} vs {tuple(b.shape)})")
        am = [getattr(a, "_glf_amax", None), getattr(b, "_glf_amax", None)]
        (ar, lda), (br, ldb) = _rows_view(a), _rows_view(b)
        for t, src, h in ((ar, a, am[0]), (br, b, am[1])):          # a copy made for the kernel keeps the source's known maximum
            if t is not src and h is not None and h[0] == src._version:
                set_amax(t, h[2])
        ca, cb = int(a.shape[-1]), int(b.shape[-1])
        rows = a.numel() // ca
        y = torch.empty(tuple(a.shape[:-1]) + (ca + cb,), dtype=a.dtype, device=a.device)
        _launch("concat2_fwd", y, ar, lda, br, ldb, y, rows, ca, cb)
        amax_bound(y, [ar, br])                             # the larger of the two sources' maxima
        ctx.cfg = (tuple(a.shape), tuple(b.shape), rows, ca, cb)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        ashape, bshape, rows, ca, cb = ctx.cfg
        dy = _contig(dy)
        da = torch.empty(ashape, dtype=dy.dtype, device=dy.device)
        db = torch.empty(bshape, dtype=dy.dtype, device=dy.device)
        _launch("concat2_bwd", dy, dy, da, db, rows, ca, cb)
        return da, db


def concat_channels(a, b):
    return ConcatChannelsFn.apply(a, b)


# ----------------------------------------------------------------------------------------
# the view mix of the classical fusion baselines (ours.py:2251-2383; csrc/view_mix.hip)
# ----------------------------------------------------------------------------------------
VIEW_MIX_MAX_V, VIEW_MIX_MAX_C, VIEW_MIX_MAX_VC = 8, 8, 40
VIEW_MIX_WGRAD_ROWS = 1024             # VM_WGRAD_ROWS: consecutive rows one workgroup reduces in wgrad
_view_mix_cache = {}


def view_mix_stack(weights, biases):
    """The operands of glf_view_mix_*: the V Conv2d weights [c, V c, 1, 1] stacked by rows into Wm [V c][V c]
    (Wm[v c + o][u c + i] = W_v[o][u c + i]) and the V biases into bm [V c].  A pure index permutation, on any device."""
    c, vc = int(weights[0].shape[0]), int(weights[0].shape[1])
    if len(weights) != len(biases) or len(weights) * c != vc or any(tuple(w.shape) != (c, vc, 1, 1) for w in weights) \
            or any(tuple(b.shape) != (c,) for b in biases):
        raise RuntimeError(f"view_mix: {len(weights)} weights of shape [c, V c, 1, 1] and as many biases [c] expected "
                           f"(got {[tuple(w.shape) for w in weights]}, {[tuple(b.shape) for b in biases]})")
    return torch.cat([w.detach().reshape(c, vc) for w in weights], dim=0), torch.cat([b.detach() for b in biases], dim=0)


def _view_mix_images(weights, biases):
    """view_mix_stack on the device as registered weight images, like fusion._qkv_weights: the two buffers live as long as the first
    weight, every row block is a GLF_WJ_COPY image of its parameter -- rebuilt when that parameter's version moved, or by
    refresh_weights().  The blocks are c * V c (and c) floats long, in general no multiple of the 16 bytes glf_copy_frames moves: a
    stale block is brought up to date by a device-to-device copy."""
    w0 = weights[0]
    c, vc = int(w0.shape[0]), int(w0.shape[1])
    key = id(w0)
    params = list(weights) + list(biases)
    hit = _view_mix_cache.get(key)
    if (hit is None or hit[0]() is not w0 or hit[1].device != w0.device or tuple(hit[1].shape) != (vc, vc)
            or any(r() is not t for r, t in zip(hit[1]._glf_sources, params))):
        view_mix_stack(weights, biases)                                  # the shape checks
        Wm = torch.empty(vc, vc, dtype=torch.float32, device=w0.device)
        bm = torch.empty(vc, dtype=torch.float32, device=w0.device)
        Wm._glf_sources = [weakref.ref(t) for t in params]
        hit = _view_mix_cache[key] = (weakref.ref(w0, lambda _r, k=key: _view_mix_cache.pop(k, None)), Wm, bm)
    _, Wm, bm = hit
    for i, (w, b) in enumerate(zip(weights, biases)):
        for t, dst, n in ((w, Wm[i * c:(i + 1) * c], c * vc), (b, bm[i * c:(i + 1) * c], c)):
            src = _contig(_chk(t, "view_mix weight").detach())
            im, fresh = _wimage(t, "viewmix", WJ_COPY, src, (n, 0, 0), lambda dst=dst: dst)
            if im.dst.data_ptr() != dst.data_ptr():       # the stacked buffers were re-created: re-register
                _registry(t.device).drop(im.key)
                im, fresh = _wimage(t, "viewmix", WJ_COPY, src, (n, 0, 0), lambda dst=dst: dst)
            if fresh:
                im.dst.copy_(src.view(im.dst.shape))
    return Wm, bm


def _ptr_table(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _view_mix_operand(t: torch.Tensor, name: str, shape=None) -> torch.Tensor:
    _chk(t, name)
    if not t.is_contiguous():
        raise RuntimeError(f"glfusion_amd: {name} must be contiguous (got strides {tuple(t.stride())} for shape {tuple(t.shape)})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"glfusion_amd: {name} has shape {tuple(t.shape)}, the first view {tuple(shape)}")
    return t if t.data_ptr() % 16 == 0 else t.clone()      # a slice that starts inside a 16-byte piece


class ViewMixFn(Function):
    """y_v = fc[v](torch.cat(xs, dim=1)) for every view v in ONE launch (glf_view_mix_fwd); the concatenation is never made.
    apply(V, x_0 .. x_{V-1}, W_0 .. W_{V-1}, b_0 .. b_{V-1}) -> V outputs."""

    @staticmethod
    def forward(ctx, v: int, *args):
        xs, weights, biases = args[:v], args[v:2 * v], args[2 * v:]
        c = int(weights[0].shape[0])
        if v > VIEW_MIX_MAX_V or c > VIEW_MIX_MAX_C or v * c > VIEW_MIX_MAX_VC:
            raise RuntimeError(f"view_mix: the limit is c <= {VIEW_MIX_MAX_C}, V <= {VIEW_MIX_MAX_V}, V * c <= {VIEW_MIX_MAX_VC} (got V = {v}, c = {c})")
        xs = [_view_mix_operand(t, "view_mix input", xs[0].shape) for t in xs]
        if c != 1 and int(xs[0].shape[-1]) != c:
            raise RuntimeError(f"view_mix: channels-last inputs [..., {c}] expected, got shape {tuple(xs[0].shape)}")
        Wm, bm = _view_mix_images(weights, biases)
        rows = xs[0].numel() // c
        ys = [torch.empty_like(xs[0]) for _ in range(v)]
        check(lib.glf_view_mix_fwd(_ptr_table(xs), _p(Wm), _p(bm), _ptr_table(ys), rows, v, c, _stream()), "view_mix_fwd")
        ctx.save_for_backward(*xs)
        ctx.cfg = (v, c, rows, Wm)
        return tuple(ys)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        xs = ctx.saved_tensors
        v, c, rows, Wm = ctx.cfg
        dev = xs[0].device
        dys = [_view_mix_operand(_contig(d), "view_mix grad", xs[0].shape) if d is not None else zeros(xs[0].shape, device=dev) for d in dys]
        need = ctx.needs_input_grad
        dxs = [None] * v
        if any(need[1:1 + v]):                              # early_fusion's inputs are data: no dgrad launch
            dxs = [torch.empty_like(xs[0]) for _ in range(v)]
            check(lib.glf_view_mix_dgrad(_ptr_table(dys), _p(Wm), _ptr_table(dxs), rows, v, c, _stream()), "view_mix_dgrad")
            dxs = [d if n else None for d, n in zip(dxs, need[1:1 + v])]
        dws, dbs = [None] * v, [None] * v
        if any(need[1 + v:]):
            vc = v * c
            dw = torch.empty(vc, vc, dtype=torch.float32, device=dev)
            db = torch.empty(vc, dtype=torch.float32, device=dev)
            nbytes = int(lib.glf_view_mix_wgrad_workspace(rows, v, c))
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            check(lib.glf_view_mix_wgrad(_ptr_table(xs), _ptr_table(dys), _p(dw), _p(db), _p(ws), nbytes, rows, v, c, _stream()), "view_mix_wgrad")
            dws = [dw[i * c:(i + 1) * c].view(c, vc, 1, 1) if need[1 + v + i] else None for i in range(v)]
            dbs = [db[i * c:(i + 1) * c] if need[1 + 2 * v + i] else None for i in range(v)]
        return (None, *dxs, *dws, *dbs)


def view_mix(xs: Sequence[torch.Tensor], weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """[fc_v(torch.cat(xs, dim=1)) for v] for V per-view Conv2d(V c, c, 1) with the weights [c, V c, 1, 1] and biases [c] as they sit
    in the modules.  xs: V contiguous fp32 tensors of one shape with the c channels innermost ([N,h,w,c]; any shape for c = 1, as
    an [N,1,H,W] image is its own channels-last form).  Limits: c <= 8, V <= 8, V c <= 40."""
    v = len(xs)
    if v == 0 or len(weights) != v or len(biases) != v:
        raise RuntimeError(f"view_mix: {v} inputs, {len(weights)} weights, {len(biases)} biases")
    return list(ViewMixFn.apply(v, *xs, *weights, *biases))


class AvgPoolFn(Function):
    """AdaptiveAvgPool2d(1): [N,H,W,C] -> fp32 [N,1,1,C].  From a bf16 map too: the ASPP pooled branch (deeplabv3.py:123-135) stays
    fp32 up to its broadcast -- its BatchNorm normalises over the N per-frame averages, which differ by less than a few bf16 steps."""

    @staticmethod
    def forward(ctx, x, lazy_grad: bool = False):
        x = _contig(_chk(x, "avgpool input", None))
        n, h, w, c = x.shape
        y = torch.empty(n, 1, 1, c, dtype=torch.float32, device=x.device)
        _launch("avgpool_fwd", x, x, y, n, h * w, c)
        ctx.cfg = (n, h, w, c, x.dtype)
        # lazy_grad: the caller guarantees that the gradient goes straight to a fan_out node, which adds the broadcast into the
        # other branch's gradient in place (glf_bcast_rows_add) -- it is handed over as a stride-0 view, never materialised
        ctx.lazy = bool(lazy_grad) and x.dtype == torch.float32 and c % 4 == 0
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        n, h, w, c, xdt = ctx.cfg
        dy = _contig(dy)
        if ctx.lazy:
            # the 1 / (h w) factor goes into the data ([N][C], one tiny launch): a consumer that does not see the tag below
            # materialises the stride-0 view and still gets the right gradient, at the price of the pass the tag saves
            ds = torch.empty(n, 1, 1, c, dtype=torch.float32, device=dy.device)
            _launch("bcast_rows_scaled", ds, dy, ds, c, 1.0 / (h * w), n, 1, c)
            dx = ds.expand(n, h, w, c)
            dx._glf_bcast = (ds, 1.0, n, h * w, c)
            return dx, None
        dx = torch.empty(n, h, w, c, dtype=xdt, device=dy.device)
        _launch("bcast_rows_scaled", dx, dy, dx, c, 1.0 / (h * w), n, h * w, c)
        return dx, None


def global_avgpool(x, lazy_grad: bool = False):
    return AvgPoolFn.apply(x, lazy_grad)


class BroadcastFn(Function):
    """bilinear up-sampling from a 1x1 map == broadcast: [N,1,1,C] -> [N,H,W,C] (into the pending output view).  Under 16-bit storage
    the input is fp32 (the pooled branch) or bf16 and the output bf16."""

    @staticmethod
    def forward(ctx, x, h: int, w: int):
        x = _contig(_chk(x, "broadcast input", None))
        n, c = x.shape[0], x.shape[-1]
        y, ldy, shared = _take_out((n, h, w, c), x.device, BF if _S16[0] else x.dtype)
        _launch("bcast_rows_scaled", y, x, y, ldy, 1.0, n, h * w, c)
        if shared is not None:                   # the broadcast repeats x: its maximum is the source's
            src = amax_of(x)
            if src is not None:
                torch.maximum(shared, src, out=shared)
            set_amax(y, shared)
        ctx.cfg = (n, h, w, c, x.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        n, h, w, c, xdt = ctx.cfg
        dy, lddy = _rows_view(dy)
        dx = torch.empty(n, 1, 1, c, dtype=xdt, device=dy.device)
        _launch("sum_rows_fwd", dy, dy, lddy, dx, 1.0, n, h * w, c)
        return dx, None, None


def broadcast_hw(x, h: int, w: int):
    return BroadcastFn.apply(x, h, w)


class FanOutFn(Function):
    """Identity with k outputs; backward sums the k incoming gradients in ONE pass (k reads + 1 write) instead of
    autograd's pairwise accumulation (3 (k-1) tensor passes through torch's add kernel)."""

    @staticmethod
    def forward(ctx, x, k: int, lazy: bool = False):
        ctx.k = k
        # lazy only when x really is a batch_norm_act output: its backward is the one node that understands `_glf_addend`
        ctx.lazy = bool(lazy) and k == 2 and LAZY_FAN_IN and type(x.grad_fn).__name__ in ("BatchNormActFnBackward", "BatchNormAct16FnBackward")
        outs = tuple(x.view_as(x) for _ in range(k))
        am = amax_of(x)                       # one measurement (or the producer's by-product) serves every alias
        share = [None]                        # ... and so does one pre-split image, whichever consumer makes it first
        for t in outs:
            set_amax(t, am)
            t._glf_pack_share = share
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        lazy = [d for d in dys if d is not None and getattr(d, "_glf_bcast", None) is not None]
        if lazy:
            # a per-frame row broadcast (AvgPoolFn, lazy_grad): added in place into the one dense gradient when this node owns it
            # (AsppCentreFn's fresh input gradient), written out as a tensor of its own otherwise
            dense = [d for d in dys if d is not None and getattr(d, "_glf_bcast", None) is None]
            own = len(dense) == 1 and getattr(dense[0], "_glf_owned", False) and dense[0].is_contiguous() and not _is16(dense[0])
            mat = []
            for d in lazy:
                src, scale, n, p, c = d._glf_bcast
                out = dense[0] if own else torch.empty(d.shape, dtype=torch.float32, device=src.device)
                check((lib.glf_bcast_rows_add if own else lib.glf_bcast_rows_scaled)(_p(src), _p(out), c, scale, n, p, c, _stream()), "bcast_rows")
                mat.append(out)
            if own:
                dense[0]._glf_amax = None        # the maximum the contractions reported no longer bounds it
                return dense[0], None, None
            dys = tuple(dense) + tuple(mat)
        live = [_contig(d) for d in dys if d is not None]
        if not live:
            return None, None, None
        if len(live) == 1:
            return live[0], None, None
        if ctx.lazy and live[0].shape == live[1].shape and not packed_only(live[0]) and not packed_only(live[1]):
            # the producer of x is a BatchNorm(+residual) whose backward adds the two while reading them (glf_bn_bwd dy2): the
            # caller of fan_out(lazy=True) guarantees that node is the ONLY reader of this gradient
            a = live[0]
            a._glf_addend = live[1]
            return a, None, None
        out = torch.empty_like(live[0])
        n = out.numel()
        w = 8 if _is16(out) else 4                # elements per 16-byte access
        if n % w != 0 or any(d.shape != out.shape for d in live) or len(live) > 8:
            raise RuntimeError(f"fan_out: gradients must share one shape with numel % {w} == 0 (<= 8 branches)")
        arr = (C.c_void_p * len(live))(*[d.data_ptr() for d in live])
        _launch("add_n", out, arr, len(live), out, n)
        return out, None, None


# The two gradients of a residual block's input go to the previous block's last BatchNorm unsummed (glf_bn_bwd adds them while reading)
LAZY_FAN_IN = os.environ.get("GLF_LAZY_FAN_IN", "1") != "0"


def fan_out(x: torch.Tensor, k: int, lazy: bool = False):
    """k aliases of x for k consumers (use each exactly once).  lazy (k == 2): the caller guarantees that x is the output of a
    batch_norm_act call and that this fan_out is its ONLY reader -- the backward then hands the two incoming gradients to that
    BatchNorm's backward as a pair (first + `_glf_addend`) instead of summing them in a pass of its own."""
    if k <= 1 or not (torch.is_grad_enabled() and x.requires_grad):
        return tuple(x for _ in range(max(k, 1)))
    return FanOutFn.apply(x, k, lazy)


# ----------------------------------------------------------------------------------------
# independent sections on side streams
# ----------------------------------------------------------------------------------------
# The per-view encoders / heads and the two fusion blocks are independent chains.  Each kernel of a chain either
# fills the chip with MFMA work in whole "rounds" of 256 workgroups (leaving the last round partly idle) or is a
# short HBM-bound pass; running the chains on separate HIP streams lets the hardware fill one chain's idle CUs
# with another chain's workgroups.  Backward nodes run on the stream their forward ran on (autograd does that), so
# the overlap carries over.  GLF_STREAMS=0 serialises everything on the current stream.
STREAMS = os.environ.get("GLF_STREAMS", "1") != "0"
N_SIDE_STREAMS = int(os.environ.get("GLF_SIDE_STREAMS", "24"))
if STREAMS and hasattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch"):
    # parameters' AccumulateGrad nodes live on the stream that first touched them (the default one when a gradient
    # hook keeps them alive); gradients produced on a side stream are synchronised into it, which is intended
    torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
_side = {}


def _walk_tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _walk_tensors(v)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            yield from _walk_tensors(v)


# True (engine.StepGraph sets it): the stream counter restarts only at begin_step() (the models call it at the top of forward),
# so successive top-level parallel_sections calls of one forward get DIFFERENT side streams instead of re-using 0, 1, 2 ...
SECTIONS_DISTINCT = False


_step_counters = {}


def step_counter(dev) -> torch.Tensor:
    """Device uint64 (held as int64) that advance_step() moves once per captured training step; the dropout kernels mix it into their
    seed, so a step replayed from a hipGraph (whose launches carry fixed seed arguments) still draws fresh masks."""
    t = _step_counters.get(dev)
    if t is None:
        t = _step_counters[dev] = zeros(1, dtype=torch.int64, device=dev)
    return t


def begin_step(dev=None) -> None:
    """Top of a model forward: restart the side-stream assignment and decide ONCE whether this step retains pre-split images
    from forward to backward (see retain_ok)."""
    for pool in _side.values():
        if pool[2] == 0:
            pool[1] = 0
    _retain_step.clear()


def advance_step(dev) -> None:
    """Advance the device step counter (one tiny launch).  A captured training step calls it ONCE, first thing, whatever the
    number of forwards it contains -- forward and backward of a Dropout must read the same value.  Eager steps need not call
    it: their dropout seeds are drawn on the host per call."""
    check(lib.glf_counter_add(_p(step_counter(dev)), 1, _stream()), "counter_add")


def reset_capture_pools() -> None:
    """Before a hipGraph capture: drop the pre-zeroed slot pools so that the pools the captured step uses are created -- and
    zero-filled -- INSIDE the capture (a replay then starts from zeroed maxima / statistics like an eager step does)."""
    _amax_pool.clear()
    _stats_pool.clear()
    _colmax_pool.clear()


def parallel_sections(fns):
    """Run the callables as independent sections, section i on side stream i, and join them on the current
    stream.  Returns their results in order."""
    if not STREAMS or len(fns) <= 1 or not torch.cuda.is_available():
        return [f() for f in fns]
    cur = torch.cuda.current_stream()
    dev = cur.device
    pool = _side.setdefault(dev, [[], 0, 0])          # streams, next index, nesting depth
    if not pool[0]:
        pool[0] = [torch.cuda.Stream(device=dev) for _ in range(N_SIDE_STREAMS)]
    # Streams are handed out in call order, restarting with every top-level call: nested calls get streams of their
    # own and a given section lands on the SAME stream every step (the caching allocator keeps one pool per stream;
    # a wandering assignment would re-allocate every activation).  A stream shared by two sections only adds an
    # ordering between them.
    if pool[2] == 0 and not SECTIONS_DISTINCT:
        pool[1] = 0
    pool[2] += 1
    used = []
    for _ in fns:
        st = pool[0][pool[1] % N_SIDE_STREAMS]
        pool[1] += 1
        if st.cuda_stream == cur.cuda_stream:
            st = pool[0][pool[1] % N_SIDE_STREAMS]
            pool[1] += 1
        used.append(st)
    outs = []
    try:
        for s, f in zip(used, fns):
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                outs.append(f())
    finally:
        pool[2] -= 1
    for s, out in zip(used, outs):
        cur.wait_stream(s)
        for t in _walk_tensors(out):
            if t.is_cuda:
                t.record_stream(cur)       # allocated on s, consumed on cur: keep the allocator from reusing it early
    return outs


# ----------------------------------------------------------------------------------------
# local gate (ours.py:1802-1816)
# ----------------------------------------------------------------------------------------
def _gate_forward(ctx, cls, ctr, f, weight: float):
    cls, ctr, f = _contig(_chk(cls, "cls")), _contig(_chk(ctr, "ctr")), _contig(_chk(f, "f4", None))
    c = f.shape[-1]
    rows = f.numel() // c
    ncls = cls.shape[-1]
    y = torch.empty_like(f)
    a = torch.empty(rows, dtype=torch.float32, device=f.device)
    am = torch.empty(rows, dtype=torch.int32, device=f.device)
    _launch("gate_fwd", f, cls, ncls, ctr, f, y, a, am, weight, rows, c)
    amax_bound(y, [f])                                      # y = f * a with a in (0, 1)
    ctx.save_for_backward(cls, ctr, f, a, am)
    ctx.cfg = (rows, c, ncls, weight)
    return y, a


class GateFn(Function):
    @staticmethod
    def forward(ctx, cls, ctr, f, weight: float):
        return _gate_forward(ctx, cls, ctr, f, weight)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        cls, ctr, f, a, am = ctx.saved_tensors
        rows, c, ncls, weight = ctx.cfg
        dy = _contig(dy)
        df = torch.empty_like(f)
        dcls = torch.empty_like(cls)
        dctr = torch.empty_like(ctr)
        _launch("gate_bwd", f, dy, f, cls, ncls, ctr, a, am, weight, df, dcls, dctr, rows, c)
        return dcls, dctr, df, None


def local_gate(cls_logits, ctr_logits, f4, weight: float):
    return GateFn.apply(cls_logits, ctr_logits, f4, float(weight))


class AxpbyFn(Function):
    """out = a*x + b*y on tensors of one shape."""

    @staticmethod
    def forward(ctx, x, y, a: float, b: float):
        x = _contig(_chk(x, "x", None))
        y = _contig(_chk(y, "y", x.dtype))
        if x.shape != y.shape:
            raise RuntimeError("axpby: shapes differ")
        out = torch.empty_like(x)
        _launch("axpby", x, x, y, out, a, b, x.numel())
        ctx.ab = (a, b)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        a, b = ctx.ab
        d = _contig(d)
        dx = dy = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(d)
            _launch("axpby", d, d, d, dx, a, 0.0, d.numel())          # a*d + 0*d
        if ctx.needs_input_grad[1]:
            dy = torch.empty_like(d)
            _launch("axpby", d, d, d, dy, b, 0.0, d.numel())
        return dx, dy, None, None


def axpby(x, y, a: float, b: float):
    return AxpbyFn.apply(x, y, float(a), float(b))


class GateMapFn(GateFn):
    """GateFn that also hands out the gate map a = sigmoid(w * max_c sigmoid(cls) * sigmoid(ctr)) as [N,1,h,w]
    (Local_only returns it as `atten_map`, ours.py:2221-2222, 2249); the map is a non-differentiable output."""

    @staticmethod
    def forward(ctx, cls, ctr, f, weight: float):
        y, a = _gate_forward(ctx, cls, ctr, f, weight)
        n, h, w = f.shape[0], f.shape[1], f.shape[2]
        amap = a.view(n, 1, h, w).clone()
        ctx.mark_non_differentiable(amap)
        return y, amap

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, _damap):
        return GateFn.backward(ctx, dy)


def local_gate_with_map(cls_logits, ctr_logits, f4, weight: float):
    return GateMapFn.apply(cls_logits, ctr_logits, f4, float(weight))


# ----------------------------------------------------------------------------------------
# view stacking / slicing for the fusion block
# ----------------------------------------------------------------------------------------
def _frames_into(dys, n, v, h, w, c):
    """[N,V,h,w,C] gradient of V per-view outputs: frame i is dys[i], zero where a view got no gradient."""
    inner = h * w * c
    ref = next(d for d in dys if d is not None)
    dg = (zeros if any(d is None for d in dys) else torch.empty)(n, v, h, w, c, dtype=ref.dtype, device=ref.device)
    for i, d in enumerate(dys):
        if d is not None:
            _launch("copy_frames", dg, _contig(d), inner, dg[:, i], v * inner, n, inner)
    return dg


class StackViewsFn(Function):
    """[N,h,w,C] x V -> [N,V,h,w,C] (ours.py:1819-1820: unsqueeze(2) + cat(dim=2) in NCDHW terms)."""

    @staticmethod
    def forward(ctx, *xs):
        dt = BF if _is16(xs[0]) else torch.float32
        xs = [_contig(_chk(t, "view feature", dt)) for t in xs]
        n, h, w, c = xs[0].shape
        v = len(xs)
        if any(t.shape != xs[0].shape for t in xs):      # the copies below take every view at the first one's extents
            raise RuntimeError(f"glfusion_amd: the views of one batch must have one shape, got {[tuple(t.shape) for t in xs]} "
                               "(the same number of frames in every view)")
        out = torch.empty(n, v, h, w, c, dtype=xs[0].dtype, device=xs[0].device)
        inner = h * w * c
        amax_bound(out, xs)                  # known BEFORE the copy: the largest of the views' maxima (fp32 storage only)
        am = getattr(out, "_glf_amax", None)
        am = am[2] if am is not None else None
        if am is not None and presplit_ok(out, am) and retain_ok(out.device):
            # the stack is read by the fusion block's contractions through its packed image only: write it in the same pass
            pk = torch.empty_like(out)
            for i, t in enumerate(xs):
                check(lib.glf_copy_frames_split(_p(t), inner, _p(out[:, i]), _p(pk[:, i]), v * inner, n, inner, _p(am), _stream()), "stack_views")
            out._glf_packed = (out._version, out.data_ptr(), am, pk, torch.cuda.current_stream() if STREAMS else None)
        else:
            for i, t in enumerate(xs):
                _launch("copy_frames", out, t, inner, out[:, i], v * inner, n, inner)
        ctx.cfg = (n, v, h, w, c)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        n, v, h, w, c = ctx.cfg
        dy = _contig(dy)
        inner = h * w * c
        outs = []
        for i in range(v):
            g = torch.empty(n, h, w, c, dtype=dy.dtype, device=dy.device)
            _launch("copy_frames", dy, dy[:, i], v * inner, g, inner, n, inner)
            outs.append(g)
        return tuple(outs)


def stack_views(xs: Sequence[torch.Tensor]):
    return StackViewsFn.apply(*xs)


class AddViewsFn(Function):
    """f4_fusion[v] = G[:, i] + L[:, i] for every view i of two [N,V,h,w,C] tensors
    (ours.py:1833-1834); returns V contiguous [N,h,w,C] tensors."""

    @staticmethod
    def forward(ctx, g, l):
        g = _contig(_chk(g, "global", None))
        l = _contig(_chk(l, "local", g.dtype))
        n, v, h, w, c = g.shape
        inner = h * w * c
        outs = []
        for i in range(v):
            out = torch.empty(n, h, w, c, dtype=g.dtype, device=g.device)
            _launch("add_frames", g, g[:, i], v * inner, l[:, i], v * inner, out, inner, n, inner)
            amax_bound(out, [g, l], sum_=True)
            outs.append(out)
        ctx.cfg = (n, v, h, w, c)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        dg = _frames_into(dys, *ctx.cfg)
        return dg, dg


def add_views(g, l):
    return AddViewsFn.apply(g, l)


class SplitViewsFn(Function):
    """[N,V,h,w,C] -> V contiguous [N,h,w,C] tensors (`conv_feat[:, :, i]` + `.contiguous()` of ours.py:2097, 2104)."""

    @staticmethod
    def forward(ctx, g):
        g = _contig(_chk(g, "stacked views", None))
        n, v, h, w, c = g.shape
        inner = h * w * c
        outs = []
        for i in range(v):
            out = torch.empty(n, h, w, c, dtype=g.dtype, device=g.device)
            _launch("copy_frames", g, g[:, i], v * inner, out, inner, n, inner)
            outs.append(out)
        ctx.cfg = (n, v, h, w, c)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        return _frames_into(dys, *ctx.cfg)


def split_views(g):
    return SplitViewsFn.apply(g)


# ----------------------------------------------------------------------------------------
# bilinear up-sampling to NCHW logits, loss, metrics
# ----------------------------------------------------------------------------------------
class BilinearUpFn(Function):
    """F.interpolate(mode='bilinear', align_corners=False): [N,h,w,C] -> NCHW [N,C,H,W]."""

    @staticmethod
    def forward(ctx, x, ho: int, wo: int):
        x = _contig(_chk(x, "upsample input"))
        n, h, w, c = x.shape
        y = torch.empty(n, c, ho, wo, dtype=torch.float32, device=x.device)
        check(lib.glf_bilinear_up_fwd(_p(x), _p(y), n, h, w, c, ho, wo, _stream()), "bilinear_up_fwd")
        ctx.cfg = (n, h, w, c, ho, wo)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        n, h, w, c, ho, wo = ctx.cfg
        dy = _contig(_chk(dy, "upsample grad"))
        dx = torch.empty(n, h, w, c, dtype=torch.float32, device=dy.device)
        check(lib.glf_bilinear_up_bwd(_p(dy), _p(dx), n, h, w, c, ho, wo, _stream()), "bilinear_up_bwd")
        return dx, None, None


def bilinear_up(x, ho: int, wo: int):
    if _is16(x):
        from . import ops16
        x = ops16.to_f32(x)
    return BilinearUpFn.apply(x, ho, wo)


class BceSumFn(Function):
    """nn.BCEWithLogitsLoss(reduction='sum') (main.py:87)."""

    @staticmethod
    def forward(ctx, logits, target):
        logits, target = _contig(_chk(logits, "logits")), _contig(_chk(target, "target"))
        if logits.shape != target.shape:
            raise RuntimeError("bce: logits/target shape mismatch")
        loss = torch.empty(1, dtype=torch.float64, device=logits.device)
        check(lib.glf_bce_logits_sum(_p(logits), _p(target), _p(loss), None, 1.0, None, logits.numel(), _stream()), "bce_logits_sum")
        ctx.save_for_backward(logits, target)
        return loss[0].float()

    @staticmethod
    @once_differentiable
    def backward(ctx, dl):
        logits, target = ctx.saved_tensors
        dx = torch.empty_like(logits)
        scratch = torch.empty(1, dtype=torch.float64, device=logits.device)
        dl = _contig(dl.float())
        # dx = (sigmoid(x) - t) * upstream, the upstream scalar read on the device (no host sync)
        check(lib.glf_bce_logits_sum(_p(logits), _p(target), _p(scratch), _p(dx), 1.0, _p(dl), logits.numel(), _stream()), "bce_logits_bwd")
        return dx, None


def bce_with_logits_sum(logits, target):
    return BceSumFn.apply(logits, target)


class CpsBceFn(Function):
    """Cross pseudo supervision (glf_cps_bce_sum): sum BCE(a, on(b)) + sum BCE(b, on(a)) with on(x) = sigmoid(x) > 0.5, the
    prediction overlap_counts scores.  The labels are constants: no gradient passes through the threshold."""

    @staticmethod
    def forward(ctx, a, b, stats):
        a, b = _contig(_chk(a, "cps logits a")), _contig(_chk(b, "cps logits b"))
        if a.shape != b.shape:
            raise RuntimeError("cps_bce_sum: the two logit maps differ in shape")
        if stats is not None and not (isinstance(stats, torch.Tensor) and stats.is_cuda and stats.dtype == torch.int64
                                      and stats.numel() == 4 and stats.is_contiguous()):
            raise RuntimeError("cps_bce_sum: stats must be a contiguous CUDA(HIP) int64 tensor of 4 elements")
        loss = torch.empty(1, dtype=torch.float64, device=a.device)
        check(lib.glf_cps_bce_sum(_p(a), _p(b), _p(loss), _p(stats), None, None, 1.0, None, a.numel(), _stream()), "cps_bce_sum")
        ctx.save_for_backward(a, b)
        return loss[0].float()

    @staticmethod
    @once_differentiable
    def backward(ctx, dl):
        a, b = ctx.saved_tensors
        da, db = torch.empty_like(a), torch.empty_like(b)
        scratch = torch.empty(1, dtype=torch.float64, device=a.device)
        dl = _contig(dl.float())
        # both gradients in one launch, the upstream scalar read on the device (no host sync)
        check(lib.glf_cps_bce_sum(_p(a), _p(b), _p(scratch), None, _p(da), _p(db), 1.0, _p(dl), a.numel(), _stream()), "cps_bce_bwd")
        return (da if ctx.needs_input_grad[0] else None), (db if ctx.needs_input_grad[1] else None), None


def cps_bce_sum(a, b, stats: Optional[torch.Tensor] = None):
    """fp32 scalar sum_i bce(a_i, on(b_i)) + bce(b_i, on(a_i)) of two fp32 logit maps of one shape (predictions are fp32 under every
    precision).  `stats`: an int64[4] device tensor the forward fills with the counts of (on(a), on(b)) = 11, 10, 01, 00."""
    return CpsBceFn.apply(a, b, stats)


def overlap_counts(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """int64 [tp, fp, fn, tn] of pred = sigmoid(logits) > 0.5 against target (main.py:800-815)."""
    logits, target = _contig(_chk(logits, "logits")), _contig(_chk(target, "target"))
    counts = torch.empty(4, dtype=torch.int64, device=logits.device)
    check(lib.glf_overlap_counts(_p(logits), _p(target), _p(counts), logits.numel(), _stream()), "overlap_counts")
    return counts


def overlap_metrics_from_counts(counts: torch.Tensor, eps: float = 1e-5):
    """(pixel_acc, dice, precision, specificity, recall) exactly as main.py:807-813."""
    tp, fp, fn, tn = [float(v) for v in counts.tolist()]
    return ((tp + tn) / (tp + tn + fp + fn + eps), (2 * tp) / (2 * tp + fp + fn + eps),
            tp / (tp + fp + eps), tn / (tn + fp + eps), tp / (tp + fn + eps))


# ----------------------------------------------------------------------------------------
# ----------------------------------------------------------------------------------------
# temporal cycle-consistency loss (main.py:213-235, 650-798)
# ----------------------------------------------------------------------------------------
class SumHWFn(Function):
    """x [..., h, w, C] channels-last (any number of leading frame dims) -> sum over (h, w): [..., C].
    `f4_global_fusion[v].sum(dim=(2, 3))` of main.py:226."""

    @staticmethod
    def forward(ctx, x):
        x = _contig(_chk(x, "sum_hw input"))
        *lead, h, w, c = x.shape
        n = 1
        for d in lead:
            n *= d
        y = torch.empty(*lead, c, dtype=torch.float32, device=x.device)
        check(lib.glf_sum_rows_fwd(_p(x), c, _p(y), 1.0, n, h * w, c, _stream()), "sum_hw")
        ctx.cfg = (tuple(x.shape), n, h * w, c)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        shape, n, p, c = ctx.cfg
        dy = _contig(dy)
        dx = torch.empty(shape, dtype=torch.float32, device=dy.device)
        check(lib.glf_bcast_rows_scaled(_p(dy), _p(dx), c, 1.0, n, p, c, _stream()), "sum_hw_bwd")
        return dx


def sum_hw(x: torch.Tensor) -> torch.Tensor:
    if _is16(x):                          # the cycle loss works on fp32 features (main.py:226): one cast of the pooled block's input
        from . import ops16
        x = ops16.to_f32(_contig(x))
    return SumHWFn.apply(x)


def pooled_fusion_features(f4_fusion: dict) -> dict:
    """{view: [T, C]} = f4_fusion[view].sum(dim=(2, 3)) (main.py:226) for the dict Global_and_Local.forward returns.
    Its entries are per-view slices of ONE [T, V, h, w, C] block (the fusion module's output): the block is pooled
    once (one read, and one broadcast in backward) instead of V strided reductions through sliced views."""
    views = list(f4_fusion)
    base = getattr(f4_fusion[views[0]], "_glf_stack", None)
    if base is not None and all(getattr(f4_fusion[v], "_glf_stack", (None, -1))[0] is base[0] for v in views):
        pooled = sum_hw(base[0])                                   # [T, V, C]
        return {v: pooled[:, f4_fusion[v]._glf_stack[1]] for v in views}
    return {v: sum_hw(to_nhwc(f4_fusion[v])) for v in views}


class SegCycleFn(Function):
    @staticmethod
    def forward(ctx, feat, target_region: int, cyc_off: int, chunk_size: int, temperature: float, start0: int, n_starts: int,
                stride: int, weight: float, soft: bool):
        feat = _contig(_chk(feat, "cycle features"))
        if feat.dim() != 2:
            raise RuntimeError("seg_cycle: features must be [T, F]")
        t, f = feat.shape
        loss = torch.empty((), dtype=torch.float32, device=feat.device)
        dfeat = torch.empty_like(feat) if ctx.needs_input_grad[0] else None
        check(lib.glf_seg_cycle(_p(feat), t, f, target_region, cyc_off, chunk_size, float(temperature), start0, n_starts, stride,
                                float(weight), int(soft), _p(loss), _p(dfeat), _stream()), "seg_cycle")
        ctx.save_for_backward(dfeat)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        (dfeat,) = ctx.saved_tensors
        out = torch.empty_like(dfeat)
        check(lib.glf_scale(_p(dfeat), _p(out), dfeat.numel(), 1.0, _p(_contig(dloss)), _stream()), "seg_cycle_bwd")
        return out, None, None, None, None, None, None, None, None, None


def seg_cycle(feat, target_region: int = 16, cyc_off: int = 2, chunk_size: int = 3, temperature: float = 10, start: int = None):
    """Trainer.seg_cycle (main.py:650-718).  `start` is the query start frame the reference draws with
    np.random.choice(target_region - (chunk_size + cyc_off) + 1) (main.py:655); None draws it the same way."""
    n = target_region - (chunk_size + cyc_off) + 1
    if start is None:
        import numpy as np
        start = int(np.random.choice(n))
    return SegCycleFn.apply(feat, target_region, cyc_off, chunk_size, temperature, int(start), 1, 1, 1.0, False)


def dense_seg_cycle(feat, target_region: int = 16, cyc_off: int = 2, chunk_size: int = 3, temperature: float = 10,
                    soft_label: bool = False, is_overlap: bool = True):
    """Trainer.dense_seg_cycle (main.py:720-798): every start frame, averaged over the number of possible starts."""
    n = target_region - (chunk_size + cyc_off) + 1
    stride = 1 if is_overlap else chunk_size
    return SegCycleFn.apply(feat, target_region, cyc_off, chunk_size, temperature, 0, (n + stride - 1) // stride, stride, 1.0 / n,
                            bool(soft_label))


# contraction precision: "f32" = exact fp32 MFMA, "bf16x6" = split-bf16 (6 MFMAs per product),
# "f16x3" = scaled split-fp16 (3 MFMAs per product).  Host-side setting handed to the library with every call.
# "bf16" = 16-bit STORAGE (BASELINE configs 3 / 5): bf16 activations / saved tensors / activation gradients in HBM, one bf16 MFMA
# per product (glfusion_amd.ops16); the few fp32 contractions left in that mode (5- / 1-channel head logits) use the exact kernels.
PRECISIONS = ("f32", "bf16x6", "f16x3", "f16", "bf16")
# ----------------------------------------------------------------------------------------
def set_precision(mode: str) -> None:
    i = PRECISIONS.index(mode)
    _S16[0] = mode == "bf16"
    _PREC[0] = 0 if _S16[0] else i


def get_precision() -> str:
    return "bf16" if _S16[0] else PRECISIONS[_PREC[0]]


class precision_scope:
    """`with ops.precision_scope("f32"): ...` -- forward AND backward of whatever runs inside must both happen inside
    the block (backward launches read the setting when they run)."""

    def __init__(self, mode: str):
        self.mode = mode

    def __enter__(self):
        self.prev = get_precision()
        set_precision(self.mode)
        return self

    def __exit__(self, *exc):
        set_precision(self.prev)
        return False
