"""Per-kernel probe of the fusion-block tail backward (profiles/tail_bwd_fused.txt): HIP events around each library call, median of 10
after 3, at 150 528 and 37 632 rows x 2048 (dqkv: x 3072).  Run from the repository root: python profiles/ubench/tail_bwd_probe.py OUT.json
(GLF_LIB_PATH selects another build; the entry points of this change are skipped where the library lacks them)."""
import sys, os, json
sys.path.insert(0, os.getcwd())
import torch
from glfusion_amd._lib import lib
DEV = torch.device("cuda:0")

def timeit(fn, n=10, warm=3):
    for _ in range(warm): fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return 0.5 * (ts[len(ts) // 2] + ts[(len(ts) - 1) // 2])

out = {}
new = hasattr(lib.load(), "glf_bn_res_ln_bwd_sums")
for rows in (150528, 37632):
    c, c3 = 2048, 3072
    T = rows * c * 4 / 1e9
    g = torch.Generator(device=DEV).manual_seed(1)
    dz = torch.randn(rows, c, device=DEV, generator=g); w = torch.randn(rows, c, device=DEV, generator=g); x = torch.randn(rows, c, device=DEV, generator=g)
    v = {k: torch.rand(c, device=DEV, generator=g) + 0.5 for k in ("mean", "invstd", "gamma", "beta", "ln_g", "ln_b")}
    z = torch.empty(rows, c, device=DEV); rmu = torch.empty(rows, device=DEV); rrs = torch.empty(rows, device=DEV)
    P = lambda t: t.data_ptr()
    assert lib.glf_bn_res_ln_fwd(P(w), P(x), P(v["mean"]), P(v["invstd"]), P(v["gamma"]), P(v["beta"]), P(v["ln_g"]), P(v["ln_b"]), 1e-5, P(z), P(rmu), P(rrs), rows, c, None, None) == 0
    del z
    du = torch.empty(rows, c, device=DEV); dwz = torch.empty(rows, c, device=DEV)
    o = [torch.empty(c, device=DEV) for _ in range(4)]; keep = torch.empty(2 * c, device=DEV)
    ws = torch.empty(int(lib.glf_bn_workspace(rows, c3)), dtype=torch.float64, device=DEV)
    am = torch.zeros(1, device=DEV)
    slot = torch.zeros(3 * c + 2, dtype=torch.float64, device=DEV)
    res = {}
    def ab():
        assert lib.glf_bn_res_ln_bwd(P(dz), P(w), P(x), P(v["mean"]), P(v["invstd"]), P(v["gamma"]), P(v["beta"]), P(v["ln_g"]), P(rmu), P(rrs), P(du), P(o[0]), P(o[1]), rows, c, P(ws), None) == 0
    res["a+b glf_bn_res_ln_bwd (du + LN colreduce + finalize)"] = (timeit(ab), 7 * T)
    def cd():
        slot.zero_(); am.zero_()
        assert lib.glf_bn_bwd(P(du), c, P(w), c, None, c, P(v["mean"]), P(v["invstd"]), P(v["gamma"]), None, P(dwz), c, None, c, P(o[2]), P(o[3]), rows, c, 0, 1, None, P(am), 1, None, None, 0, P(slot), None) == 0
    res["c+d glf_bn_bwd fused form packed (atomic reduce + apply)"] = (timeit(cd), 5 * T)
    def c2():
        am.zero_()
        assert lib.glf_bn_bwd(P(du), c, P(w), c, None, c, P(v["mean"]), P(v["invstd"]), P(v["gamma"]), None, P(dwz), c, None, c, P(o[2]), P(o[3]), rows, c, 0, 1, P(ws), P(am), 2, None, None, 0, P(keep), None) == 0
    res["(c') glf_bn_bwd packed_dx=2 (two-stage reduce + finalize)"] = (timeit(c2), 2 * T)
    def d3():
        assert lib.glf_bn_bwd(P(du), c, P(w), c, None, c, P(v["mean"]), P(v["invstd"]), P(v["gamma"]), None, P(dwz), c, None, c, None, None, rows, c, 0, 1, P(ws), P(am), 3, None, None, 0, P(keep), None) == 0
    res["d glf_bn_bwd packed_dx=3 (apply alone)"] = (timeit(d3), 3 * T)
    if new:
        def A():
            am.zero_()
            assert lib.glf_bn_res_ln_bwd_sums(P(dz), P(w), P(x), P(v["mean"]), P(v["invstd"]), P(v["gamma"]), P(v["beta"]), P(v["ln_g"]), P(rmu), P(rrs), P(du), P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(keep), P(am), rows, c, 1, P(ws), None) == 0
        res["A glf_bn_res_ln_bwd_sums (walk + finalize)"] = (timeit(A), 4 * T)
    del dz, w, x, du, dwz
    dq = torch.randn(rows, c3, device=DEV, generator=g); pk = torch.empty_like(dq); s = torch.empty(c3, device=DEV)
    amq = dq.abs().max().reshape(1)
    Q = rows * c3 * 4 / 1e9
    res["e glf_split_f16_packed dqkv"] = (timeit(lambda: lib.glf_split_f16_packed(P(dq), rows, c3, c3, P(amq), P(pk), c3, None)), 2 * Q)
    res["f glf_colsum dqkv"] = (timeit(lambda: lib.glf_colsum(P(dq), c3, P(s), rows, c3, P(ws), None)), Q)
    if new:
        res["E glf_split_f16_packed_colsum dqkv"] = (timeit(lambda: lib.glf_split_f16_packed_colsum(P(dq), rows, c3, c3, P(amq), P(pk), c3, P(s), P(ws), None)), 2 * Q)
    del dq, pk
    for k, (ms, gb) in res.items():
        print(f"rows {rows:6d}  {k:62s} {ms:7.3f} ms  {gb / ms * 1e3 / 1e3:6.2f} TB/s ({gb:.2f} GB)", flush=True)
    out[rows] = {k: [ms, gb] for k, (ms, gb) in res.items()}
    torch.cuda.empty_cache()
json.dump(out, open(sys.argv[1], "w"), indent=1)
