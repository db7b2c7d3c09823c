#!/usr/bin/env python3
"""BatchNorm streaming passes at the flagship shapes (fp32 storage, f16x3): HIP events around each library call, median of 10 after
3, time and algorithmic GB/s, with add_n (two addends) on a tensor of the same size beside it -- the rate this access pattern is
known to reach.  A/B of two builds: run once per build with GLF_LIB_PATH.

  bn_stream_probe.py [--save DIR | --compare DIR] [--pair-only]

  --save DIR      also write every output of the apply kernels (fp32, packed image, sign bytes, coefficients) to DIR/*.npy, inputs
                  from fixed seeds
  --compare DIR   compare the same outputs bit for bit with what --save wrote (another build) and say so per tensor
  --pair-only     only the backward reduce + apply pair at 50176 x 256 and 50176 x 1024 (the Infinity Cache order experiment)

Modes (what the model runs at these shapes):
  fwd inner    glf_bn_apply_from_sums, ReLU, packed image out (colmax), no residual           8 B / element
  fwd last     glf_bn_apply_from_sums, residual + ReLU + sign bytes, fp32 out                  12.25 B / element
  bwd inner    glf_bn_bwd two launches, sign recomputed from x, packed dx                      20 B / element (8 reduce + 12 apply)
  bwd last     glf_bn_bwd two launches, dy + dy2, sign bytes, dres, packed dx                  32.5 B / element re-adding the pair in
               the apply pass, 28.25 B with the masked sum written once by the reduce pass: both rates are printed
  bwd apply    the apply pass alone (packed_dx = 3 on sums kept by a packed_dx = 2 call), sign recomputed, packed dx   12 B / element
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from glfusion_amd import ops                                   # noqa: E402
from glfusion_amd._lib import lib, check                       # noqa: E402

DEV = torch.device("cuda", 0)
SHAPES = [(193600, 64), (193600, 256), (50176, 256), (50176, 512), (50176, 1024), (50176, 2048)]
EPS, MOM = 1e-5, 0.1


def p(t):
    return None if t is None else t.data_ptr()


def rnd(rows, c, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(rows, c, generator=g, device=DEV) * (2.0 * scale) - scale + shift


def timed(fn, reset=None, n=10, warm=3):
    ts = []
    for i in range(warm + n):
        if reset is not None:
            reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts), max(ts) - min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save")
    ap.add_argument("--compare")
    ap.add_argument("--pair-only", action="store_true")
    args = ap.parse_args()
    ops.set_precision("f16x3")
    print(f"library: {os.environ.get('GLF_LIB_PATH', 'default')}")
    keep_dir = args.save or args.compare
    if args.save:
        os.makedirs(args.save, exist_ok=True)
    mismatches = []

    def record(tag, **tensors):
        if not keep_dir:
            return
        for name, t in tensors.items():
            path = os.path.join(keep_dir, f"{tag}_{name}.npy")
            a = t.detach().cpu().contiguous().view(torch.uint8).numpy()
            if args.save:
                np.save(path, a)
            else:
                same = np.array_equal(np.load(path), a)
                print(f"    {tag} {name}: {'bit-identical' if same else 'DIFFERS'}")
                if not same:
                    mismatches.append(f"{tag} {name}")

    shapes = [(50176, 256), (50176, 1024)] if args.pair_only else SHAPES
    for rows, c in shapes:
        n = rows * c
        x = rnd(rows, c, 1, 2.0, 0.3)
        res = rnd(rows, c, 2)
        dy, dy2 = rnd(rows, c, 3, 3.0), rnd(rows, c, 4, 0.7)
        gamma, beta = rnd(1, c, 5, 0.5, 1.0).view(c), rnd(1, c, 6).view(c)
        sums = torch.stack([x.double().sum(0), (x.double() ** 2).sum(0)]).contiguous()
        colmax = x.abs().amax(0).contiguous()
        y, pk, dx, dres = (torch.empty(rows, c, device=DEV) for _ in range(4))
        mask = torch.empty(rows * (c // 4), dtype=torch.uint8, device=DEV)
        mean, invstd = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        rm, rv, nbt = torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
        am = torch.zeros(1, device=DEV)
        dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        fs = torch.zeros(3 * c, dtype=torch.float64, device=DEV)
        keep = torch.empty(2 * c, device=DEV)
        ws = torch.empty(int(lib.glf_bn_workspace(rows, c)), dtype=torch.float64, device=DEV)
        print(f"rows x C = {rows} x {c}  ({n * 4 / 1e6:.0f} MB per fp32 tensor)")

        def report(name, bytes_per_el, t, spread, alt=None):
            extra = f"   ({alt * n / t / 1e6:7.0f} GB/s at {alt} B / element)" if alt else ""
            print(f"  {name:44s} {t * 1e3:8.1f} us  spread {spread * 1e3:5.1f}  {bytes_per_el * n / t / 1e6:7.0f} GB/s at {bytes_per_el} B / element{extra}")

        def fwd_inner():
            check(lib.glf_bn_apply_from_sums(p(x), c, None, c, p(pk), c, p(sums), rows, c, EPS, MOM, p(gamma), p(beta), p(mean), p(invstd),
                                             p(rm), p(rv), p(nbt), 1, p(am), None, p(colmax), None), "fwd inner")

        def fwd_last():
            check(lib.glf_bn_apply_from_sums(p(x), c, p(res), c, p(y), c, p(sums), rows, c, EPS, MOM, p(gamma), p(beta), p(mean), p(invstd),
                                             p(rm), p(rv), p(nbt), 1, p(am), p(mask), None, None), "fwd last")

        def bwd_inner():
            check(lib.glf_bn_bwd(p(dy), c, p(x), c, None, c, p(mean), p(invstd), p(gamma), p(beta), p(dx), c, None, c, p(dg), p(db),
                                 rows, c, 1, 1, None, p(am), 1, None, None, 0, p(fs), None), "bwd inner")

        def bwd_last():
            check(lib.glf_bn_bwd(p(dy), c, p(x), c, None, c, p(mean), p(invstd), p(gamma), p(beta), p(dx), c, p(dres), c, p(dg), p(db),
                                 rows, c, 1, 1, None, p(am), 1, p(mask), p(dy2), c, p(fs), None), "bwd last")

        def bwd_phase(phase):
            check(lib.glf_bn_bwd(p(dy), c, p(x), c, None, c, p(mean), p(invstd), p(gamma), p(beta), p(dx), c, None, c,
                                 p(dg) if phase == 2 else None, p(db) if phase == 2 else None,
                                 rows, c, 1, 1, p(ws), p(am), phase, None, None, 0, p(keep), None), "bwd phase")

        def zero():
            fs.zero_(); am.zero_()

        arr = (C.c_void_p * 2)(dy.data_ptr(), dy2.data_ptr())

        def add_n():
            check(lib.glf_add_n(arr, 2, p(dres), n, None), "add_n")

        if not args.pair_only:
            am.zero_(); fwd_inner(); torch.cuda.synchronize()
            record(f"{rows}x{c}_fwd_inner", image=pk, bound=am, mean=mean, invstd=invstd, rmean=rm, rvar=rv)
            report("fwd inner (packed out)", 8, *timed(fwd_inner, am.zero_))
            am.zero_(); fwd_last(); torch.cuda.synchronize()
            record(f"{rows}x{c}_fwd_last", y=y, mask=mask, amax=am, mean=mean, invstd=invstd)
            report("fwd last (residual, ReLU, sign bytes)", 12.25, *timed(fwd_last, am.zero_))
            zero(); bwd_inner(); torch.cuda.synchronize()
            record(f"{rows}x{c}_bwd_inner", image=dx)           # (bound, dgamma, dbeta come from f64 atomics: no fixed order)
            report("bwd inner pair (packed dx)", 20, *timed(bwd_inner, zero))
        zero(); fwd_last(); zero(); bwd_last(); torch.cuda.synchronize()
        record(f"{rows}x{c}_bwd_last", dres=dres)
        report("bwd last pair (dy + dy2, bytes, dres, packed)", 32.5, *timed(bwd_last, zero), alt=28.25)
        if not args.pair_only:
            am.zero_(); bwd_phase(2); bwd_phase(3); torch.cuda.synchronize()
            record(f"{rows}x{c}_bwd_apply", image=dx, bound=am)
            report("bwd apply alone (packed dx)", 12, *timed(lambda: bwd_phase(3)))
            report("add_n, two addends", 12, *timed(add_n))
        del x, res, dy, dy2, y, pk, dx, dres, ws
        torch.cuda.empty_cache()
    if args.compare:
        print("bit-identity against the saved outputs: " + ("ALL bit-identical" if not mismatches else f"{len(mismatches)} differ: {mismatches}"))


if __name__ == "__main__":
    main()
