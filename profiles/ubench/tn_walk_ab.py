#!/usr/bin/env python3
"""Bitwise A/B of two builds of the library over the TN kernels' tap pick, slice walk, row state, store epilogue and second stage
(csrc/gemm_tn_walk.h).

For each case of a fixed list the call runs on seeded inputs and a SHA-256 of the bytes of C (and of amax_c where requested) is
printed: every case of tests/test_gpu_tn_walk.py under f32, bf16x6, f16x3 and f16, the bf16-storage TN cases of
tests/test_gpu_s16_gemm.py (TN_PLAIN, TN_GATHER; both C dtypes) and the VARIANTS of tests/test_gpu_tn_reduce_oihw.py.  Every one
of them is reproducible from run to run (the two-stage path has no atomics, `accumulate` at split 1 adds once per element,
atomicMax is order-free), so every case is compared bit for bit.

Usage: tn_walk_ab.py                     one run of the library GLF_LIB_PATH (or the tree's) selects
       tn_walk_ab.py LIB_A LIB_B         two fresh child processes one after the other, then the comparison"""
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
    from glfusion_amd import ops
    import test_gpu_tn_walk as W
    import test_gpu_s16_gemm as S
    import test_gpu_tn_reduce_oihw as O

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]

    def out(name, prec, what):
        print(f"CASE {name} {prec} {what}", flush=True)

    for prec in W.PRECISIONS:
        with ops.precision_scope(prec):
            for case in W.CASES + (W.AMAX_CASES if prec == "f16x3" else []):
                c, _, slot = W.run_case(ops, case)
                out(case["name"], prec, f"sha C {sha(c)}" + (f" amax {sha(slot)}" if slot is not None else ""))
    for prec in ("f32", "f16x3"):
        with ops.precision_scope(prec):
            for n, h, w, cin, cout, split in O.VARIANTS:
                dy, x = O._operands(n, h, w, cin, cout)
                dw = O._fused(ops, dy, x, cin, cout, O._kw(n, h, w, cin, cout, 1, (1 << 9) - 1, split, False))
                torch.cuda.synchronize()
                out(f"oihw_{n}x{h}x{w}_{cin}_{cout}_s{split}", prec, f"sha C {sha(dw)}")
    with ops.precision_scope("bf16"):
        for name, s in list(S.TN_PLAIN.items()) + list(S.TN_GATHER.items()):
            M, N, K, batch, taps = s["M"], s["N"], s["K"], s["batch"], s["taps"]
            src = S.src_index(1, s["geo"]) if s["conv"] is not None else torch.arange(K).view(1, K)
            mask = (S.mask_of(src) if s["conv"] is not None else 1) if s["mask"] is None else s["mask"]
            live = S.kept_taps(mask, taps)
            A, B = S.operand("gauss", (batch, K, M), 11, K), S.operand("gauss", (batch, s["rows_b"], N), 12, K)
            dA = S.Frame((batch, K, M), (s["bsa"], s["lda"], 1), S.BF).put(A).upload()
            dB = S.Frame((batch, s["rows_b"], N), (s["bsb"], s["ldb"], 1), S.BF).put(B).upload()
            for cdt in (S.BF, S.F32):
                fc = S.Frame((batch, taps, M, N), (s["bsc"], s["tsb"], s["ldc"], 1), cdt)
                fc.idx = fc.idx[:, live]
                S.call16("tn", dA, dB, fc.upload(), M=M, N=N, K=K, lda=s["lda"], ldb=s["ldb"], ldc=s["ldc"], taps=taps, mask=mask, tap_stride_b=s["tsb"],
                         gather=s["gather"], geo=s["geo"], batch=batch, bsa=s["bsa"], bsb=s["bsb"], bsc=s["bsc"], alpha=S.f32_alpha(s["alpha_g"]),
                         split=s["split"], rect=s["rect"])
                out(f"s16_{name}_{'bf16' if cdt == S.BF else 'fp32'}C", "bf16", f"sha C {sha(fc.result(name))}")


def run(lib):
    env = dict(os.environ)
    if lib:
        env["GLF_LIB_PATH"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, HERE, "child"], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-4000:])
        sys.exit(2 if p.returncode > 0 else 128 - p.returncode)      # (1 is kept for "digests differ"; a signal shows as 128 + its number)
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
            bad += not same
            print(f"{k[0]:44s} {k[1]:6s} bitwise   {'same' if same else 'DIFFERENT'}  A: {a[k]}" + ("" if same else f"  B: {b.get(k)}"))
        print(f"{len(a)} cases, {bad} different")
        sys.exit(1 if bad else 0)
    else:
        for k, v in run(os.environ.get("GLF_LIB_PATH")).items():
            print(f"{k[0]:44s} {k[1]:6s} {v}")
