#!/usr/bin/env python3
"""Bitwise A/B of two builds of the library over the NT kernels' tile walk, row state and epilogue (csrc/gemm_rows_walk.h).

For each case of a fixed list the call runs on seeded inputs through ops.gemm (f32, bf16x6, f16x3 and f16; the first two skip
what only the split-fp16 kernels build: column statistics, the fused epilogue, region mode, pre-split operands) or the
bf16-storage NT entry point and a SHA-256 of the bytes of C (and of amax_c where requested) is printed.  Two kinds of case are not bitwise
reproducible from run to run -- per-tap rectangles (rect = 1: float atomics into C) and column statistics fed by more than
one row tile (f64 atomics across workgroups) -- and are compared against float64 instead (the elementwise 5e-5 of
tests/test_gpu_ops.py for C, 1e-6 relative for the statistics).

Usage: rows_walk_ab.py                     one run of the library GLF_LIB_PATH (or the tree's) selects
       rows_walk_ab.py LIB_A LIB_B         two fresh child processes one after the other, then the comparison
GLF_AB_PRECISIONS=f32,bf16x6 restricts the list to those precisions (default: all five)."""
import hashlib
import os
import subprocess
import sys

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from glfusion_amd import ops, ops16
    from test_gpu_rows_walk import NO_CENTRE, REGION_MASK, geo_of, src_index, gathered_ref, rnd, close
    dev = torch.device("cuda", 0)

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]

    def out(name, prec, what):
        print(f"CASE {name} {prec} {what}", flush=True)

    def plain(name, prec, M, N, K, bias=False, accumulate=False, colstats=False, bitwise=True, epi=False):
        A, B = rnd(M, K, seed=1), rnd(N, K, seed=2)
        bi = rnd(N, seed=3) if (bias or epi) else None
        c = rnd(M, N, seed=4).to(dev) if accumulate else torch.empty(M, N, device=dev)
        ref = A.double() @ B.double().T + (bi.double() if bi is not None else 0.0) + (c.double().cpu() if accumulate else 0.0)
        kw = {}
        if colstats:
            kw = dict(colstats=torch.zeros(2, N, dtype=torch.float64, device=dev), colmax=torch.zeros(N, device=dev), amax_c=ops.amax_slot(dev))
        if epi:
            res = rnd(M, N + 8, seed=5)
            kw["epilogue"] = (res.to(dev), N + 8, True)
            ref = torch.relu(ref + res[:, :N].double())
        ops.gemm("nt", A.to(dev), B.to(dev), c, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bi.to(dev) if bi is not None else None,
                 accumulate=accumulate, **kw)
        torch.cuda.synchronize()
        if colstats and not bitwise:
            got = c.double().cpu()
            ok = (close(c, ref, 5e-5 if prec == "f16x3" else 2e-2) and torch.allclose(kw["colstats"][0].cpu(), got.sum(0), rtol=1e-6, atol=1e-6 * float(got.abs().sum(0).max()))
                  and torch.allclose(kw["colstats"][1].cpu(), (got * got).sum(0), rtol=1e-6) and torch.equal(kw["colmax"].cpu(), c.abs().amax(0).cpu()))
            out(name, prec, f"f64 C {sha(c)} amax {sha(kw['amax_c'])} stats-ok {int(ok)}")
        elif colstats:
            out(name, prec, f"sha C {sha(c)} stats {sha(kw['colstats'])} colmax {sha(kw['colmax'])} amax {sha(kw['amax_c'])}")
        else:
            out(name, prec, f"sha C {sha(c)}")

    def gathered(name, prec, gather, conv, K, N, mask, rect=0, accumulate=False):
        geo = geo_of(gather, conv)
        M, rows_a = geo[0] * geo[3] * geo[4], geo[0] * geo[1] * geo[2]
        A, B = rnd(rows_a, K, seed=11), rnd(9, N, K, seed=12) / 3
        cold = rnd(M, N, seed=13) if accumulate else torch.zeros(M, N)
        c = cold.to(dev).clone()
        ops.gemm("nt", A.to(dev), B.to(dev), c, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, taps=9, mask=mask, tap_stride_b=N * K, gather=gather,
                 geo=geo, rect=rect, accumulate=accumulate)
        torch.cuda.synchronize()
        if rect == 1:
            ref = gathered_ref(A, B, src_index(gather, geo), mask)
            out(name, prec, f"f64 ok {int(close(c, ref, 2e-2 if prec == 'f16' else 5e-5))}")
        else:
            out(name, prec, f"sha C {sha(c)}")

    def nn(name, prec, conv, K, N, mask, rect=0, bias=False):
        """C = sum_t A[src_t] @ B_t, B [taps][K][N]: the exact kernel's BMODE = 1, whatever the precision; conv None = plain"""
        geo = geo_of(2, conv) if conv else None
        M, rows_a, taps = (geo[0] * geo[3] * geo[4], geo[0] * geo[1] * geo[2], 9) if conv else (129, 129, 1)
        A, B = rnd(rows_a, K, seed=31), rnd(taps, K, N, seed=32) / 3
        bi = rnd(N, seed=33) if bias else None
        c = torch.zeros(M, N, device=dev)
        ops.gemm("nn", A.to(dev), B.to(dev), c, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, bias=bi.to(dev) if bias else None, taps=taps, mask=mask,
                 tap_stride_b=K * N, gather=2 if conv else 0, geo=geo, rect=rect)
        torch.cuda.synchronize()
        if rect == 1:
            out(name, prec, f"f64 ok {int(close(c, gathered_ref(A, B.transpose(1, 2), src_index(2, geo), mask), 5e-5))}")
        else:
            out(name, prec, f"sha C {sha(c)}")

    wanted = [p for p in os.environ.get("GLF_AB_PRECISIONS", "f32,bf16x6,f16x3,f16,bf16").split(",") if p]
    for prec in [p for p in ("f32", "bf16x6", "f16x3", "f16") if p in wanted]:
        ops.set_precision(prec)
        split16 = prec in ("f16x3", "f16")
        for K, tile in ((32, 128), (288, 256)):
            for N in (132, 70):
                plain(f"plain_m{tile + 1}_n{N}_k{K}_bias", prec, tile + 1, N, K, bias=True)
                plain(f"plain_m{tile + 1}_n{N}_k{K}_accumulate", prec, tile + 1, N, K, accumulate=True)
            plain(f"grouped_m{4 * tile + 1}_n900_k{K}", prec, 4 * tile + 1, 900, K)
            if split16:
                plain(f"colstats_m{2 * tile + 3}_k{K}", prec, 2 * tile + 3, 132, K, bias=True, colstats=True, bitwise=False)
                plain(f"colstats_m{tile - 5}_k{K}_one_tile", prec, tile - 5, 132, K, bias=True, colstats=True)
                plain(f"epi_m{tile + 1}_n132_k{K}", prec, tile + 1, 132, K, epi=True)
        for K in (32, 64):
            for g in (1, 2):
                gathered(f"census_g{g}_k{K}", prec, g, (1, 28, 28, 3, 1, 12, 12), K, 72, NO_CENTRE)
                if split16:
                    gathered(f"region_g{g}_k{K}_accumulate", prec, g, (1, 28, 28, 3, 1, 12, 12), K, 72, REGION_MASK[g], rect=2, accumulate=True)
                gathered(f"rect1_g{g}_k{K}", prec, g, (1, 28, 28, 3, 1, 24, 24), K, 72, NO_CENTRE, rect=1)
            gathered(f"dgrad_s2_k{K}", prec, 2, (1, 55, 55, 3, 2, 1, 1), K, 72, NO_CENTRE)
        if not split16:
            # what the split-fp16 precisions never reach: a K tail (every precision's fallback to the exact kernel), three images
            # of a non-square map, and the NN form of the exact kernel
            plain("plain_m129_n70_k33_bias", prec, 129, 70, 33, bias=True)
            for g in (1, 2):
                gathered(f"census_3img_g{g}_k32", prec, g, (3, 28, 20, 3, 1, 12, 12), 32, 72, 0x1FF)
                gathered(f"rect1_3img_g{g}_k32", prec, g, (3, 28, 20, 3, 1, 12, 12), 32, 72, 0x1FF, rect=1)
            gathered("dgrad_s2_2img_k33", prec, 2, (2, 23, 23, 3, 2, 1, 1), 33, 72, 0x1FF)
            nn("nn_plain_k33_bias", prec, None, 33, 70, 1, bias=True)
            nn("nn_census_3img_k32", prec, (3, 28, 20, 3, 1, 12, 12), 32, 72, 0x1FF)
            nn("nn_dgrad_s2_k32", prec, (1, 55, 55, 3, 2, 1, 1), 32, 72, NO_CENTRE)
            nn("nn_rect1_3img_k32", prec, (3, 28, 20, 3, 1, 12, 12), 32, 72, 0x1FF, rect=1)
        # the model's own shapes (f16s4_probe.py): plain projections with pre-split weights, activations pre-split or not
        g = torch.Generator(device=dev).manual_seed(0)
        drnd = lambda *s: torch.rand(*s, device=dev, generator=g) * 2 - 1
        for M, N, K in [(193600, 256, 64), (193600, 64, 256), (193600, 64, 64), (50176, 512, 128), (50176, 128, 512), (50176, 1024, 256),
                        (50176, 256, 1024), (50176, 2048, 512), (50176, 512, 2048), (50176, 256, 1280), (50176, 256, 2048), (150528, 3072, 2048)]:
            if not split16 and M * N * K > 1 << 36:
                continue                                   # the largest one takes the exact kernel 20 s
            A, B, c = drnd(M, K), drnd(N, K), torch.empty(M, N, device=dev)
            if not split16:
                ops.gemm("nt", A, B, c, M=M, N=N, K=K, lda=K, ldb=K, ldc=N)
                torch.cuda.synchronize()
                out(f"model_nt_{M}_{N}_{K}", prec, f"sha C {sha(c)}")
                del A, B, c
                continue
            ama, amb = ops.amax_of(A), ops.amax_of(B)
            Ap, Bp = ops.packed_of(A, ama), ops.packed_of(B, amb)
            for pa in (False, True):
                ops.gemm("nt", Ap if pa else A, Bp, c, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, amax_a=ama, amax_b=amb, a_packed=pa, b_packed=True)
                torch.cuda.synchronize()
                out(f"model_nt_{M}_{N}_{K}_pa{int(pa)}", prec, f"sha C {sha(c)}")
            del A, B, c, Ap, Bp
        for nimg, hh, cin, cout, dil in [(64, 55, 64, 64, 1), (64, 28, 128, 128, 1), (64, 28, 256, 256, 2)]:
            x = drnd(nimg, hh, hh, cin).requires_grad_(True)
            w = (drnd(cout, cin, 3, 3) / (3 * cin ** 0.5)).requires_grad_(True)
            y = ops.conv2d(x, w, None, 1, dil, dil)
            y.backward(drnd(nimg, hh, hh, cout))
            torch.cuda.synchronize()
            out(f"model_conv3x3_{nimg * hh * hh}_{cout}_{cin}", prec, f"sha y {sha(y)} dx {sha(x.grad)}")
            del x, w, y
    if "bf16" not in wanted:
        return
    ops.set_precision("bf16")
    BF = torch.bfloat16

    def s16(name, M, N, K, gather=0, conv=None, rect=0, mask=1, bias=False):
        geo = geo_of(gather, conv) if gather else None
        if gather:
            M, rows_a, taps = geo[0] * geo[3] * geo[4], geo[0] * geo[1] * geo[2], 9
        else:
            rows_a, taps = M, 1
        A, B = rnd(rows_a, K, seed=21).to(BF), (rnd(taps, N, K, seed=22) / 3).to(BF)
        bi = rnd(N, seed=23).to(dev) if bias else None
        for cdt in (BF, torch.float32):
            c = torch.full((M, N), 7.0, dtype=cdt, device=dev)
            ops16.gemm16("nt", A.to(dev), B.to(dev), c, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bi, taps=taps, mask=mask, tap_stride_b=N * K,
                         gather=gather, geo=geo, rect=rect)
            torch.cuda.synchronize()
            out(f"{name}_{'bf16' if cdt == BF else 'fp32'}C", "bf16", f"sha C {sha(c)}")

    s16("s16_plain_m257_n60_k64", 257, 60, 64, bias=True)
    s16("s16_plain_m257_n128_k64", 257, 128, 64, bias=True)
    for g in (1, 2):
        s16(f"s16_census_g{g}", None, 136, 64, gather=g, conv=(1, 28, 28, 3, 1, 12, 12), mask=0x1FF)
        s16(f"s16_region_g{g}_empty_region", None, 136, 64, gather=g, conv=(1, 28, 28, 3, 1, 12, 12), rect=2, mask=REGION_MASK[g], bias=True)
    s16("s16_dgrad_s2", None, 136, 64, gather=2, conv=(1, 55, 55, 3, 2, 1, 1), mask=0x1FF)


def run(lib):
    env = dict(os.environ)
    if lib:
        env["GLF_LIB_PATH"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, HERE, "child"], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-4000:])
        sys.exit(1)
    return {tuple(l.split()[1:3]): " ".join(l.split()[3:]) for l in p.stdout.splitlines() if l.startswith("CASE ")}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
    elif len(sys.argv) == 3:
        a = run(sys.argv[1])
        b = run(sys.argv[2])
        bad = 0
        for k in a:
            same = a[k] == b.get(k)
            f64 = a[k].startswith("f64")
            if f64:              # compared against float64 in each run, not with each other
                same = a[k].endswith("ok 1") and b.get(k, "").endswith("ok 1")
            bad += not same
            print(f"{k[0]:44s} {k[1]:6s} {'f64-gated' if f64 else 'bitwise  '} {'same' if same else 'DIFFERENT'}  A: {a[k]}" + ("" if same and not f64 else f"  B: {b.get(k)}"))
        print(f"{len(a)} cases, {bad} different")
        sys.exit(1 if bad else 0)
    else:
        for k, v in run(os.environ.get("GLF_LIB_PATH")).items():
            print(f"{k[0]:44s} {k[1]:6s} {v}")
