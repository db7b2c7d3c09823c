#!/usr/bin/env python3
"""Bitwise A/B of two builds of the library over the BatchNorm column reductions and the statistics finish (csrc/col_reduce.h,
csrc/norm.hip): every instantiation of the BatchNorm-backward reduce of both storages and of the bf16 column reduce, the three
users of the statistics finish, and one ops.batch_norm_act forward + backward per storage.

One SHA-256 per case, over the bytes of every output that is reproducible from run to run.  With the integer family of
tests/s16_stream_ref.py every sum is exact, so that is everything: sums, maxima, dbeta, dgamma, dres, dx, y, mask bytes, mean,
invstd and the running statistics.  With the gaussian family the sums meet in f64 atomics in no fixed order: the digest then
covers what does not pass through them (dres, eval-mode dx, and everything of the statistics finish, whose sums are an input),
and the sums are held to the interval gate of tests/test_gpu_s16_stream.py instead ("gate 1").

Usage: bn_merge_ab.py                     one run of the library GLF_LIB_PATH (or the tree's) selects
       bn_merge_ab.py LIB_A LIB_B         two fresh child processes one after the other (the second only if the first
                                          exited 0), each under its own time limit, then the comparison"""
import hashlib
import os
import subprocess
import sys

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
CHILD_LIMIT = 420                                          # seconds per child

SHAPES = [(70, 72), (297, 136), (1031, 4096)]
CAP = {4: (4100, 4096), 8: (8500, 4096)}                   # the slice cap of red_geom<W>, per access width


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import s16_stream_ref as R
    from glfusion_amd import ops
    from glfusion_amd._lib import lib, check
    dev, F32, F64, BF = R.DEV, R.F32, R.F64, R.BF
    p = lambda t: None if t is None else t.data_ptr()

    def sha(*ts):
        h = hashlib.sha256()
        for t in ts:
            if t is not None:
                h.update(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
        return h.hexdigest()[:32]

    def out(name, what):
        print(f"CASE {name} {what}", flush=True)

    def inputs(fam, rows, c, cap):
        if not cap:
            return R.bn_inputs(fam, rows, c)
        g = torch.Generator(device=dev).manual_seed(71)
        ri = lambda lo, hi: torch.randint(lo, hi + 1, (rows, c), generator=g, device=dev).double()
        return R.Bag(R.bn_inputs("int", 5, c), x=ri(-3, 3), dy=ri(-2, 2), dy2=ri(-2, 2), res=ri(-2, 2))

    def gated(got, ref, mag, k, extra):
        d = R.tol(k, mag) + (0.0 if extra is None else extra)
        return bool(((got.double() - ref).abs() <= d).all())

    def bwd_cases(fam, rows, c, cap=False):
        """the BatchNorm-backward reduce of both storages, every instantiation (at a slice cap: the one the tests run)"""
        I = inputs(fam, rows, c, cap)
        training = int(fam == "int")
        v, vmag = R.bn_fwd_ref(I.x, I.mean, I.invstd, I.gamma, I.beta)
        vres = v + I.res
        unsure = R.unsure_of(v, vmag, R.K_V_NORES)
        pos = {1: vres > 0, 2: v > 0, 3: vres > 0}
        vec = [R.vec32(I[k]) for k in ("mean", "invstd", "gamma", "beta")]
        for w in (4, 8):
            if cap and (rows, c) != CAP[w]:
                continue
            dt = F32 if w == 4 else BF
            x, dy, dy2, y = I.x.to(dt), I.dy.to(dt), I.dy2.to(dt), torch.relu(vres).to(dt)
            rpt = R.red_geometry(rows, c, w)[4]
            # fused: the single-stage reduce with atomics; on fp32 storage also the three-launch form (two-stage reduce, no atomics)
            combos = [(True, 2, True, 0, True)] if cap else [(h2, rm, dr, pk, fu) for h2 in (False, True) for rm in range(4 if w == 4 else 3)
                                                             for dr in (False, True) for pk in ((0, 1) if w == 4 else (0,))
                                                             for fu in ((True, False) if w == 4 else (True,)) if fu or dr]
            ws = torch.empty(int(lib.glf_bn_workspace(rows, c)), dtype=F64, device=dev) if w == 4 and not cap else None
            for has2, rm, want_dres, packed, fused in combos:
                b = R.bn_bwd_ref(I.dy, I.dy2 if has2 else None, I.x, I.mean, I.invstd, None if rm == 0 else pos[rm].double())
                mask = R.sign_bytes(pos[1], w) if rm == 1 else None
                dx, dres = torch.empty(rows, c, dtype=dt, device=dev), (torch.empty(rows, c, dtype=dt, device=dev) if want_dres else None)
                dg, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
                fs = torch.zeros(3 * c, dtype=F64, device=dev)                  # 2 c doubles of sums, 2 c floats of maxima (fp32 storage)
                am = torch.zeros(1, device=dev)
                if w == 4:
                    check(lib.glf_bn_bwd(p(dy), c, p(x), c, p(y) if rm == 3 else None, c, *map(p, vec), p(dx), c, p(dres), c, p(dg), p(db), rows, c,
                                         int(rm != 0), training, None if fused else p(ws), p(am), packed, p(mask), p(dy2) if has2 else None, c,
                                         p(fs) if fused else None, None), "bn_bwd")
                else:
                    check(lib.glf_s16_bn_bwd(p(dy), c, p(dy2) if has2 else None, c, p(x), c, *map(p, vec), p(dx), c, p(dres), c, p(dg), p(db), rows, c,
                                             int(rm != 0), training, p(fs), p(mask), None), "s16_bn_bwd")
                torch.cuda.synchronize()
                name = f"bwd_w{w}_{fam}_{rows}x{c}_has2{int(has2)}_rm{rm}_dres{int(want_dres)}_packed{packed}" + ("" if fused else "_3launch")
                if not fused:                                                   # no atomics: reproducible whatever the values
                    out(name, f"sha {sha(dg, db, dres, dx, am)}")
                elif fam == "int":
                    R.assert_exact(b.s1mag, 4 * b.s2mag)
                    assert torch.equal(fs[:2 * c], torch.cat([b.s1, b.s2])), name + ": the sums are not the exact ones"
                    out(name, f"sha {sha(fs, dg, db, dres, dx, am)}")
                else:
                    e1, e2 = ((unsure * b.g0mag).sum(0), (unsure * b.g0mag * b.xhmag).sum(0)) if rm == 2 else (None, None)
                    ok = gated(db, b.s1, b.s1mag, 1 + rpt + 1, e1) and gated(dg, b.s2, b.s2mag, 4 + rpt + 1, e2)
                    out(name, f"sha {sha(fs[2 * c:], dres, dx, am)} gate {int(ok)}")

    def colreduce_cases(fam, rows, c, cap=False):
        """glf_s16_colstats and glf_s16_colsum: the two instantiations of the bf16 column reduce"""
        I = inputs(fam, rows, c, cap)
        x, dy = I.x.to(BF), I.dy.to(BF)
        sums, ws, db = torch.zeros(2, c, dtype=F64, device=dev), torch.empty(2 * c, dtype=F64, device=dev), torch.empty(c, device=dev)
        check(lib.glf_s16_colstats(p(x), c, rows, c, p(sums), None), "s16_colstats")
        check(lib.glf_s16_colsum(p(dy), c, p(db), rows, c, p(ws), None), "s16_colsum")
        if not cap:                                                             # fp32 storage: two stages, no atomics
            dy32, db32, ws32 = I.dy.float(), torch.empty(c, device=dev), torch.empty(int(lib.glf_bn_workspace(rows, c)), dtype=F64, device=dev)
            check(lib.glf_colsum(p(dy32), c, p(db32), rows, c, p(ws32), None), "colsum")
            torch.cuda.synchronize()
            out(f"colsum32_{fam}_{rows}x{c}", f"sha {sha(db32)}")
        torch.cuda.synchronize()
        ref, mag = R.colstats_ref(I.x)
        name = f"colreduce16_{fam}_{rows}x{c}"
        if fam == "int":
            R.assert_exact(mag, I.dy.abs().sum(0))
            out(name, f"sha {sha(sums, db)}")
        else:
            k = R.red_geometry(rows, c)[4]
            ok = gated(sums, ref, mag, k, None) and gated(db, I.dy.sum(0), I.dy.abs().sum(0), k + 1, None)
            out(name, f"gate {int(ok)}")

    def finish_cases(fam, rows, c):
        """glf_bn_stats, glf_bn_apply_from_sums (plain and packed) and glf_s16_bn_apply in train mode: the users of bn_finish"""
        I = R.bn_inputs(fam, rows, c)
        x32, r32, x16, r16 = I.x.float(), I.res.float(), I.x.to(BF), I.res.to(BF)
        gamma, beta = R.vec32(I.gamma), R.vec32(I.beta)
        sums = R.colstats_ref(I.x)[0].contiguous()                              # float64, an INPUT of the applies
        colmax = I.x.abs().amax(0).float()
        rm0, rv0 = R.uniform32((c,), 51, -0.1, 0.1).float().to(dev), R.uniform32((c,), 52, 0.5, 1.5).float().to(dev)
        new = lambda: (torch.empty(c, device=dev), torch.empty(c, device=dev), rm0.clone(), rv0.clone(), torch.zeros(1, dtype=torch.int64, device=dev))
        mean, invstd, rm, rv, nbt = new()
        ws = torch.empty(int(lib.glf_bn_workspace(rows, c)), dtype=F64, device=dev)
        check(lib.glf_bn_stats(p(x32), c, rows, c, R.EPS, R.MOM, p(mean), p(invstd), p(rm), p(rv), p(nbt), p(ws), None), "bn_stats")
        torch.cuda.synchronize()
        out(f"finish_bn_stats_{fam}_{rows}x{c}", f"sha {sha(mean, invstd, rm, rv, nbt)}")
        for res, relu, want_mask in ((False, False, False), (True, True, True)):
            mean, invstd, rm, rv, nbt = new()
            y, am = torch.empty(rows, c, device=dev), torch.zeros(1, device=dev)
            mask = torch.zeros(rows, c // 4, dtype=torch.uint8, device=dev) if want_mask else None
            check(lib.glf_bn_apply_from_sums(p(x32), c, p(r32) if res else None, c, p(y), c, p(sums), rows, c, R.EPS, R.MOM, p(gamma), p(beta), p(mean),
                                             p(invstd), p(rm), p(rv), p(nbt), int(relu), p(am), p(mask), None, None), "bn_apply_from_sums")
            torch.cuda.synchronize()
            out(f"finish_apply_sums_{fam}_{rows}x{c}_res{int(res)}", f"sha {sha(y, mask, am, mean, invstd, rm, rv, nbt)}")
            mean, invstd, rm, rv, nbt = new()
            y16 = torch.empty(rows, c, dtype=BF, device=dev)
            mask = torch.zeros(rows, c // 8, dtype=torch.uint8, device=dev) if want_mask else None
            check(lib.glf_s16_bn_apply(p(x16), c, p(r16) if res else None, c, p(y16), c, p(sums), rows, c, R.EPS, R.MOM, p(gamma), p(beta), p(mean),
                                       p(invstd), p(rm), p(rv), p(nbt), int(relu), p(mask), None), "s16_bn_apply")
            torch.cuda.synchronize()
            out(f"finish_s16_apply_{fam}_{rows}x{c}_res{int(res)}", f"sha {sha(y16, mask, mean, invstd, rm, rv, nbt)}")
        mean, invstd, rm, rv, nbt = new()
        y, am = torch.empty(rows, c, device=dev), torch.zeros(1, device=dev)
        check(lib.glf_bn_apply_from_sums(p(x32), c, None, c, p(y), c, p(sums), rows, c, R.EPS, R.MOM, p(gamma), p(beta), p(mean), p(invstd), p(rm),
                                         p(rv), p(nbt), 1, p(am), None, p(colmax), None), "bn_apply_from_sums(packed)")
        torch.cuda.synchronize()
        out(f"finish_apply_sums_{fam}_{rows}x{c}_colmax", f"sha {sha(y, am, mean, invstd, rm, rv, nbt)}")

    def op_case(prec):
        """ops.batch_norm_act, residual and ReLU, forward and backward: 200 rows are ONE row slice at either access width, so every
        column meets one atomic and the sums are reproducible whatever their values"""
        ops.set_precision(prec)
        dt = BF if prec == "bf16" else F32
        n, h, w, c = 2, 10, 10, 136
        I = R.bn_inputs("int", n * h * w, c)
        bn = torch.nn.BatchNorm2d(c).to(dev).train()
        with torch.no_grad():
            bn.weight.copy_(I.gamma)
            bn.bias.copy_(I.beta)
        x = I.x.to(dt).view(n, h, w, c).requires_grad_(True)
        res = I.res.to(dt).view(n, h, w, c).requires_grad_(True)
        y = ops.batch_norm_act(x, bn, True, residual=res)
        y.backward(I.dy.to(dt).view(n, h, w, c))
        torch.cuda.synchronize()
        out(f"op_batch_norm_act_{prec}", f"sha {sha(y, x.grad, res.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var, bn.num_batches_tracked)}")

    ops.set_precision("f16x3")
    for fam in ("int", "gauss"):
        for rows, c in SHAPES:
            bwd_cases(fam, rows, c)
            colreduce_cases(fam, rows, c)
            finish_cases(fam, rows, c)
    for rows, c in sorted(set(CAP.values())):
        bwd_cases("int", rows, c, cap=True)
    colreduce_cases("int", *CAP[8], cap=True)
    for prec in ("f16x3", "bf16"):
        op_case(prec)


def run(lib):
    env = dict(os.environ)
    if lib:
        env["GLF_LIB_PATH"] = os.path.abspath(lib)
    p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, HERE, "child"], env=env, capture_output=True, text=True)
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-4000:])
        print(f"child with {lib or 'the default library'} exited {p.returncode}: nothing further is run")
        sys.exit(1)
    return {l.split()[1]: " ".join(l.split()[2:]) for l in p.stdout.splitlines() if l.startswith("CASE ")}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
    elif len(sys.argv) == 3:
        a = run(sys.argv[1])
        b = run(sys.argv[2])
        bad = 0
        for k in a:
            same = a[k] == b.get(k) and not a[k].endswith("gate 0")
            bad += not same
            print(f"{k:56s} {'same' if same else 'DIFFERENT'}  A: {a[k]}" + ("" if same else f"  B: {b.get(k)}"))
        bad += len(set(b) - set(a))
        print(f"{len(a)} cases, {bad} different")
        sys.exit(1 if bad else 0)
    else:
        for k, v in run(os.environ.get("GLF_LIB_PATH")).items():
            print(f"{k:56s} {v}")
