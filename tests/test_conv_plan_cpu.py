"""CPU, no library: glfusion_amd.conv_plan.plan() against the frozen table golden/conv_plan_table.json.

The table was recorded from the functions that stated the planner's rules before it existed (ops.tap_mask / rect_fraction / region_mode /
_rect_thr / wgrad_split, ops16._region / tn_split16 and the conditions written out in Conv2dFn, _conv_wgrad, AsppCentreFn, fold_plan,
Conv2d16Fn and fold_plan16; every wrapper asks the planner now), for every precision of ops.PRECISIONS, every pass and every geometry: the fifteen of
test_abi_cpu.py::test_conv_plan_matches_host_policy plus 16-bit region / rectangle cases on both sides of the rows_o >= 2048 rule,
pad != dil, stride 2 with dilation, centre tap only, a partial mask (only the middle row of taps survives) and a mask that is empty
in both directions.  Pass "fwd_bias" is the forward of a conv with a bias (what the conv does about column statistics then was
never asked: null).  The fwd_folded rows of the two precisions that have no folded Python path came from glf_conv2d_plan.
keep_rows: both semantics of `keep` with keep = ~CENTRE_TAP on the 3x3 pad == dil geometries."""
import json
import os
import subprocess
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_table.json")


def _table():
    with open(GOLDEN) as f:
        return json.load(f)


def test_planner_reproduces_the_frozen_table():
    from glfusion_amd import conv_plan
    t = _table()
    geoms = [tuple(g[:5]) + (g[5], g[5]) + tuple(g[6:]) for g in t["geometries"]]           # k -> kh, kw
    assert t["columns"] == ["prec", "pass", "geometry", "mask", "kept", "rect", "split", "zero_fill", "colstats_ok", "ho", "wo"]
    seen = set()
    for prec, pass_, gi, mask, kept, rect, split, zero_fill, colstats_ok, ho, wo in t["rows"]:
        pl = conv_plan.plan(pass_.replace("_bias", ""), geoms[gi], prec, bias=pass_.endswith("_bias"))
        got = (pl.mask, pl.kept, pl.rect, pl.split, pl.zero_fill, pl.colstats_ok if colstats_ok is not None else None, pl.ho, pl.wo)
        assert got == (mask, kept, rect, split, zero_fill, colstats_ok, ho, wo), (t["precisions"][prec], pass_, geoms[gi], got)
        seen.add((prec, pass_, gi))
    assert len(seen) == len(t["rows"]) == len(t["precisions"]) * 5 * len(geoms) and len(t["precisions"]) == 5
    keep = ~conv_plan.CENTRE_TAP
    assert t["keep"] == keep & 0x1ff and t["keep_columns"] == ["prec", "pass", "geometry", "mask", "kept", "rect", "split", "zero_fill"]
    same = [g for g in geoms if g[5] == 3 and g[7] == 1 and g[8] == g[9]]
    assert len(t["keep_rows"]) == 4 * 3 * len(same)                                            # fp32 storage: the callers of keep
    for prec, pass_, gi, mask, kept, rect, split, zero_fill in t["keep_rows"]:
        pl = conv_plan.plan(pass_, geoms[gi], prec, keep)
        assert (pl.mask, pl.kept, pl.rect, pl.split, pl.zero_fill) == (mask, kept, rect, split, zero_fill), (t["precisions"][prec], pass_, geoms[gi], pl)


def test_plan_fields_are_consistent():
    from glfusion_amd import conv_plan
    t = _table()
    for g in t["geometries"]:
        n, h, w, cin, cout, k, stride, pad, dil = g
        geom = (n, h, w, cin, cout, k, k, stride, pad, dil)
        for pass_ in conv_plan.PASSES:
            pl = conv_plan.plan(pass_, geom, 2)
            assert pl.taps == k * k and pl.kept == bin(pl.mask).count("1") and pl.plain == (k == 1 and stride == 1 and pad == 0)
            assert (pl.geo is None) == pl.plain and pl.gather == (0 if pl.plain else 2 if pass_ == "dgrad" else 1)
            rows_o, rows_i = n * pl.ho * pl.wo, n * h * w
            assert (pl.M, pl.N, pl.K) == {"dgrad": (rows_i, cin, cout), "wgrad": (cout, cin, rows_o)}.get(pass_, (rows_o, cout, cin))
            if not pl.plain:
                src, dst = ((pl.ho, pl.wo), (h, w)) if pass_ == "dgrad" else ((h, w), (pl.ho, pl.wo))
                assert pl.geo == (n,) + src + dst + (k, k, stride, pad, dil)
            assert pl.split == 1 or pass_ == "wgrad"
            assert pl.workspace_bytes == (pl.split * pl.kept * cout * cin * 4 if pl.split > 1 else 0)


def test_ops_holds_no_launch_policy_of_its_own():
    """The fp32-storage wrappers ask the planner: the policy names ops still offers ARE the planner's objects (whoever changes a
    threshold through ops changes the planner's), the helpers that restated the rules are gone, and conv_stats_fusable answers
    what the frozen table records for the forward pass under the four fp32-storage precisions."""
    import torch
    from glfusion_amd import conv_plan, ops
    assert ops.tap_mask is conv_plan.tap_mask and ops.rect_fraction is conv_plan.rect_fraction
    assert ops.RECT_THRESHOLD is conv_plan.RECT_THRESHOLD and ops.CENTRE_TAP == conv_plan.CENTRE_TAP
    for name in ("region_mode", "_rect_thr", "_conv_out", "wgrad_split", "_mask_cache", "_rect_cache"):
        assert not hasattr(ops, name), name
    t = _table()
    seen = 0
    for prec, pass_, gi, _, _, _, _, _, colstats_ok, _, _ in t["rows"]:
        if pass_ != "fwd" or t["precisions"][prec] == "bf16":
            continue
        n, h, w, cin, cout, k, stride, pad, dil = t["geometries"][gi]
        with ops.precision_scope(t["precisions"][prec]):
            got = ops.conv_stats_fusable(torch.empty(cout, cin, k, k, device="meta"), stride, pad, dil, h, w)
        assert got == colstats_ok, (t["precisions"][prec], t["geometries"][gi])
        seen += 1
    assert seen == 4 * len(t["geometries"])


def test_planner_loads_without_torch_or_the_library():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); from glfusion_amd import conv_plan, _lib; "
            "assert conv_plan.plan('fwd', (2, 28, 28, 64, 64, 3, 3, 1, 12, 12), 2).rect == 1; "
            "assert 'torch' not in sys.modules and _lib.lib._dll is None" % root)
    subprocess.run([sys.executable, "-c", code], check=True)
