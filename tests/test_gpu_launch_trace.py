"""GPU: the launches the convolution wrappers issue, against a recording.

A spy on ops.gemm and ops16.gemm16 (the way test_gpu_aspp_centre_wgrad.py wraps ops.gemm) writes down the scalar arguments of every
contraction, in order, while small workloads run: ASPP train steps (twice per model, so that retained images and the packed_hit
routes are taken), single conv2d calls forward and backward, and folded-BatchNorm inference of the same ASPPs.  The recording
(golden/launch_trace.json) was made by this module (`python tests/test_gpu_launch_trace.py --record`) at the commit before the launch
planner glfusion_amd.conv_plan existed; the module touches only ops.gemm, ops16.gemm16 and public classes, so it runs unchanged on
both sides.  The test asserts that the traces are equal: for the 16-bit-storage wrappers, which ask the planner, and for the
fp32-storage wrappers, whose move to it this recording is there to check.

The recording also holds a SHA-256 of every output and gradient, taken from several recording runs: for a case whose runs agreed in
every tensor the digests are asserted bit for bit (a plan that routes the same and sums the same gives the same bits).  A case in
which any tensor differed between runs, or in which a launch sums several taps in float atomics (per-tap rectangles, NT / NN), holds
null digests and only its trace is asserted: one such sum makes everything after it order-dependent, and a tensor that happened to
agree between the recording runs (fp16 operand rounding often hides a last-bit difference) would fail now and then."""
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_trace.json")

# (n, h, w, cin, cout, rates): the first two are shapes "a" and "c" of test_gpu_aspp_centre_wgrad.py (in "c" no branch sums with
# atomics); 16-bit storage needs Cout % 64 == 0
ASPP_SHAPES = {"a": (3, 28, 28, 64, 32, (12, 24, 36)), "c": (2, 12, 10, 64, 32, (1, 1, 12)), "s16": (2, 28, 28, 64, 64, (12, 24, 36))}
ASPP_TRAIN = [(s, p) for s in ("a", "c") for p in ("f32", "f16x3", "f16")] + [("s16", "bf16")]
ASPP_FOLDED = [("a", "f16x3"), ("c", "f16x3"), ("s16", "bf16")]
CONVS = {"3x3s1p1": (3, 1, 1, 1), "3x3s2p1": (3, 2, 1, 1), "1x1s2": (1, 2, 0, 1), "3x3p2d2": (3, 1, 2, 2)}        # k, stride, pad, dil
RECORD_RUNS = 4
CONV_IN = (2, 12, 10, 64, 64)                                                                                   # n, h, w, cin, cout
CASES = ([f"aspp_train-{s}-{p}" for s, p in ASPP_TRAIN] + [f"aspp_folded-{s}-{p}" for s, p in ASPP_FOLDED]
         + [f"conv-{g}-{b}-{p}" for p in ("f32", "f16x3", "bf16") for g in CONVS for b in ("bias", "nobias")])


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _record(trace, fn, mode, k):
    geo, seg, foreign = k.get("geo"), k.get("seg"), k.get("foreign")
    trace.append([fn, mode, k["M"], k["N"], k["K"], k["lda"], k["ldb"], k["ldc"], k.get("taps", 1), k.get("mask", 1), k.get("gather", 0),
                  None if geo is None else [int(v) for v in geo], int(k.get("split", 1)), int(k.get("rect", 0)),
                  bool(k.get("accumulate", False)), bool(k.get("a_packed", False)), bool(k.get("b_packed", False)), bool(k.get("oihw", False)),
                  None if foreign is None else int(foreign[0]), None if seg is None else [int(seg[0]), [[int(v) for v in s] for s in seg[1]]],
                  k.get("bias") is not None, k.get("colstats") is not None, k.get("amax_c") is not None, k.get("epilogue") is not None])


class _Spy:
    """Every ops.gemm / ops16.gemm16 call inside the block appends its scalar arguments to .trace."""

    def __enter__(self):
        from glfusion_amd import ops, ops16
        self.trace, self.keep = [], (ops.gemm, ops16.gemm16)

        def wrap(fn, real):
            def spy(mode, *a, **k):
                _record(self.trace, fn, mode, k)
                return real(mode, *a, **k)
            return spy
        ops.gemm, ops16.gemm16 = wrap("gemm", self.keep[0]), wrap("gemm16", self.keep[1])
        return self

    def __exit__(self, *exc):
        from glfusion_amd import ops, ops16
        ops.gemm, ops16.gemm16 = self.keep
        return False


def _fill(module, seed):
    """Parameters and running statistics from a CPU generator, in state_dict order (independent of the global RNG)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if name.endswith("num_batches_tracked"):
                t.zero_()
            elif name.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif name.endswith("running_mean") or name.endswith("bias"):
                t.copy_(torch.rand(t.shape, generator=g) - 0.5)
            elif t.dim() == 1:
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            else:
                t.copy_(torch.randn(t.shape, generator=g) / (t[0].numel() ** 0.5))


def _enter(x_nchw, prec):
    """The NHWC activation of the precision's storage dtype made from the NCHW fp32 leaf."""
    from glfusion_amd import ops, ops16
    x = ops.to_nhwc(x_nchw)
    return ops16.to_bf16(x) if prec == "bf16" else x


def _leave(y):
    from glfusion_amd import ops16
    return ops16.to_f32(y) if y.dtype == torch.bfloat16 else y


def _aspp(shape, prec, folded):
    from glfusion_amd import ops
    from glfusion_amd.models.deeplabv3 import ASPP
    n, h, w, cin, cout, rates = ASPP_SHAPES[shape]
    g = torch.Generator().manual_seed(11)
    x0, up = torch.randn(n, cin, h, w, generator=g), torch.randn(n, h, w, cout, generator=g)
    dev = torch.device("cuda:0")
    digests = {}
    switch = ops.set_fold_bn_s16 if prec == "bf16" else ops.set_fold_bn
    with ops.precision_scope(prec), _Spy() as spy:
        m = ASPP(cin, list(rates), cout)
        _fill(m, 5)
        m = m.to(dev)
        m = m.eval() if folded else m.train()
        try:
            if folded:
                switch(True)
            for step in range(2):               # the second pass finds the images the first one retained
                if folded:
                    with torch.no_grad():
                        y = _leave(m.trunk_nhwc(_enter(x0.to(dev), prec)))
                    digests[f"{step}.y"] = _digest(y)
                    continue
                for p in m.parameters():
                    p.grad = None
                x = x0.to(dev).requires_grad_(True)
                y = _leave(m.trunk_nhwc(_enter(x, prec)))          # everything up to the Dropout, which draws a fresh mask per call
                (y * up.to(dev)).sum().backward()
                torch.cuda.synchronize()
                digests[f"{step}.y"], digests[f"{step}.dx"] = _digest(y), _digest(x.grad)
                for name, p in m.named_parameters():
                    digests[f"{step}.{name}"] = _digest(p.grad)
        finally:
            if folded:
                switch(False)
        torch.cuda.synchronize()
    return {"trace": spy.trace, "digest": digests}


def _conv(geom, bias, prec):
    from glfusion_amd import ops
    n, h, w, cin, cout = CONV_IN
    k, stride, pad, dil = CONVS[geom]
    g = torch.Generator().manual_seed(13)
    dev = torch.device("cuda:0")
    x = torch.randn(n, cin, h, w, generator=g).to(dev).requires_grad_(True)
    wt = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(dev).requires_grad_(True)
    b = (torch.rand(cout, generator=g) - 0.5).to(dev).requires_grad_(True) if bias else None
    with ops.precision_scope(prec), _Spy() as spy:
        y = _leave(ops.conv2d(_enter(x, prec), wt, b, stride, pad, dil))
        up = torch.randn(y.shape, generator=g).to(dev)
        (y * up).sum().backward()
        torch.cuda.synchronize()
    digests = {"y": _digest(y), "dx": _digest(x.grad), "dw": _digest(wt.grad)}
    if bias:
        digests["db"] = _digest(b.grad)
    return {"trace": spy.trace, "digest": digests}


def run_case(case):
    kind, a, b = case.split("-", 2)
    if kind == "conv":
        bias, prec = b.split("-")
        return _conv(a, bias == "bias", prec)
    return _aspp(a, b, kind == "aspp_folded")


_EXPECTED = {}


def _expected():
    if not _EXPECTED:
        with open(GOLDEN) as f:
            _EXPECTED.update(json.load(f))
    return _EXPECTED


@pytest.mark.parametrize("case", CASES)
def test_launches_and_bits_match_the_recording(case):
    want = _expected()[case]
    got = json.loads(json.dumps(run_case(case)))               # (tuples -> lists, as the recording was read)
    assert len(got["trace"]) == len(want["trace"]), (len(got["trace"]), len(want["trace"]))
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, f"{case}: launch {i}: got {g}, recorded {w}"
    assert sorted(got["digest"]) == sorted(want["digest"])
    for name, d in want["digest"].items():
        if d is not None:                                      # null: a case whose sums depend on the order of float atomics
            assert got["digest"][name] == d, f"{case}: {name} differs in bits from the recording"


def test_the_deterministic_cases_are_pinned_bit_for_bit():
    """The atomics-free ASPP shape under f16x3 and every 16-bit-storage case carry a digest for every tensor."""
    want = _expected()
    for case in CASES:
        if case == "aspp_train-c-f16x3" or case.endswith("-bf16"):
            assert all(d is not None for d in want[case]["digest"].values()), case


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python tests/test_gpu_launch_trace.py --record")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    runs = [{c: run_case(c) for c in CASES} for _ in range(RECORD_RUNS)]
    out = {}
    for c in CASES:
        trace = json.loads(json.dumps(runs[0][c]["trace"]))
        assert all(json.loads(json.dumps(r[c]["trace"])) == trace for r in runs), f"{c}: two runs launched differently"
        atomics = any(t[13] == 1 and t[1] != "tn" and bin(t[9]).count("1") > 1 for t in trace)
        loose = sorted(k for k, v in runs[0][c]["digest"].items() if any(r[c]["digest"][k] != v for r in runs))
        pinned = not atomics and not loose
        out[c] = {"trace": trace, "digest": {k: (v if pinned else None) for k, v in runs[0][c]["digest"].items()}}
        print(f"{c}: {len(trace)} launches, {'PINNED bit for bit' if pinned else 'trace only'}: multi-tap float atomics {atomics}, "
              f"{len(loose)} of {len(runs[0][c]['digest'])} tensors differed over {RECORD_RUNS} runs" + (f" ({', '.join(loose)})" if loose else ""))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
