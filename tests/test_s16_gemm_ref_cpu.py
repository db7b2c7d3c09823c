"""CPU: the references, preconditions, gates and case tables of tests/test_gpu_s16_gemm.py (which is a GPU module as a whole).

The gates must have teeth before they judge a kernel: the per-element interval accepts an fp32-accumulate, round-to-nearest-even
result and rejects the same result stored by truncation or with one 16-deep k-step removed; the integer gate rejects both as well;
the gather-index references agree with F.conv2d and its autograd in float64; the case tables reach every kernel variant and path
(computed with the host formulas of gemm_s16.hip)."""
import math

import torch

import test_gpu_s16_gemm as T

BF, F32 = torch.bfloat16, torch.float32


def test_bf16_rounding_helpers_pin_ties_to_even():
    x = torch.tensor([256.0, 257.0, 258.0, 259.0, 261.0, 511.0, -257.0, -259.0], dtype=torch.float64)
    assert T.bf16_rne(x).tolist() == [256.0, 256.0, 258.0, 260.0, 260.0, 512.0, -256.0, -260.0]
    assert T.bf16_trunc(x.float()).tolist() == [256.0, 256.0, 258.0, 258.0, 260.0, 510.0, -256.0, -258.0]
    assert T.f32_alpha(1.0 / 49) == float(torch.tensor(1.0 / 49, dtype=F32)) != 1.0 / 49


def _torch_result(A, B, alpha, drop_step=False):
    acc = T.nt_emulate(A, B, torch.arange(A.shape[0]).view(1, -1), 1)
    if drop_step:
        acc = (acc.double() - A[:, 32:48] @ B[0][:, 32:48].T).float()
    return (acc.double() * alpha).float()


def test_interval_gate_accepts_rne_rejects_truncation_and_dropped_step():
    M, N, K = 300, 200, 512
    A, B = T.gauss((M, K), 1), T.gauss((1, N, K), 2)
    alpha = T.f32_alpha(1.0 / 49)
    src = torch.arange(M).view(1, M)
    P, Q = T.nt_products(A, B, src, 1)
    ref, absref = alpha * P, abs(alpha) * Q
    good = _torch_result(A, B, alpha)
    for c_bf16, store in ((True, lambda v: v.to(BF)), (False, lambda v: v)):
        bad, worst = T.interval_violations(store(good), ref, absref, K, c_bf16)
        assert int(bad.sum()) == 0 and (c_bf16 or worst < 1.0)
        T.gate_interval(store(good), ref, absref, K, c_bf16, "correct result")
        dropped, _ = T.interval_violations(store(_torch_result(A, B, alpha, drop_step=True)), ref, absref, K, c_bf16)
        assert int(dropped.sum()) > 0.5 * M * N                      # one of 32 k-steps missing: most elements leave the interval
    trunc, _ = T.interval_violations(T.bf16_trunc(good).to(BF), ref, absref, K, True)
    assert int(trunc.sum()) > 0.1 * M * N                            # measured: about a fifth of the elements
    # the whole-tensor gates of test_gpu_s16.py accept that truncating store: this is the gap the interval closes
    assert T.rel_l2(T.bf16_trunc(good), ref) <= 4e-3
    T.gate_emulation(good, good, ref, "emulation against itself")


def test_integer_gate_rejects_truncation_dropped_step_and_one_wrong_element():
    M, N, K = 64, 72, 512
    A, B = T.dense_ints((M, K), 3), T.dense_ints((1, N, K), 4)
    P, Q = T.nt_products(A, B, torch.arange(M).view(1, M), 1)
    T.assert_exact_precondition(2.0 * Q + 64)
    good = _torch_result(A, B, -2.0)
    assert torch.equal(good.double(), -2.0 * P)                        # every partial sum is exact, whatever the order
    T.gate_exact(good, -2.0 * P, False, "fp32")
    T.gate_exact(good.to(BF), -2.0 * P, True, "bf16")
    ties = ((P.abs() * 2 >= 256) & (P.abs() * 2 < 512) & (P % 2 == 1)).sum()
    assert int(ties) >= 0
    for wrong in (T.bf16_trunc(good).to(BF), _torch_result(A, B, -2.0, drop_step=True).to(BF)):
        try:
            T.gate_exact(wrong, -2.0 * P, True, "bf16")
        except AssertionError:
            continue
        raise AssertionError("the integer gate accepted a wrong result")
    one = good.clone()
    one[17, 5] += 1.0
    try:
        T.gate_exact(one, -2.0 * P, False, "fp32")
    except AssertionError:
        pass
    else:
        raise AssertionError("the integer gate accepted one wrong element")
    try:
        T.assert_exact_precondition(torch.tensor([2.0 ** 24]))
    except AssertionError:
        pass
    else:
        raise AssertionError("precondition accepted 2^24")


def test_dense_integer_results_contain_bf16_ties():
    """odd integers in [256, 512) (and their scaled kin) are exact ties: the dense family does pin ties-to-even"""
    s = T.NT_PLAIN["m1100_n384_k2048"]
    A, B = T.dense_ints((s["M"], s["K"]), 1), T.dense_ints((1, s["N"], s["K"]), 2)
    P, _ = T.nt_products(A, B, torch.arange(s["M"]).view(1, -1), 1)
    ties = (T.bf16_rne(P) != P) & ((P.abs() >= 256) & (P.abs() < 512) & (P.abs() % 2 == 1))
    assert int(ties.sum()) > 100
    assert not torch.equal(T.bf16_rne(P), T.bf16_trunc(P.float()).double())


def test_ternary_family_stays_in_the_exact_range_of_the_statistics():
    for n_terms in (64, 2048, 2304):
        a, b = T.ternary((200, n_terms), 5, n_terms), T.ternary((120, n_terms), 6, n_terms)
        assert float((a.abs() @ b.abs().T).max()) <= 255
        assert abs(float(a.abs().mean()) - min(0.5, math.sqrt(96.0 / n_terms))) < 0.02


def test_gather_index_references_agree_with_conv2d_and_autograd():
    for conv in ((2, 9, 7, 3, 1, 2, 2), (2, 9, 9, 3, 2, 1, 1), (1, 14, 14, 3, 2, 1, 1), (2, 8, 6, 1, 2, 0, 1), (1, 10, 12, 3, 1, 12, 12)):
        n, h, w, k, stride, pad, dil = conv
        cin, cout = 8, 16
        g1, g2 = T.geo_of(1, conv), T.geo_of(2, conv)
        ho, wo = g1[3], g1[4]
        x, dy = T.dense_ints((n * h * w, cin), 7), T.dense_ints((n * ho * wo, cout), 8)
        W = T.dense_ints((k * k, cout, cin), 9)
        s1, s2 = T.src_index(1, g1), T.src_index(2, g2)
        assert torch.equal(T.nt_products(x, W, s1, T.mask_of(s1))[0], T.conv_fwd_ref(x, W, conv))
        WT = W.transpose(1, 2).contiguous()
        assert torch.equal(T.nt_products(dy, WT, s2, T.mask_of(s2))[0], T.conv_dgrad_ref(dy, WT, conv))
        m = T.mask_of(s1)
        live = T.kept_taps(m, k * k)
        assert torch.equal(T.tn_products(dy, x, s1, m)[0][live], T.conv_wgrad_ref(dy, x, conv)[live])
        # rectangle enumeration = the in-range rows in ascending order; the emulations reproduce the exact integer result
        emu = T.tn_emulate(dy, x, s1, m, 0.5, 3, 1)
        assert torch.equal(emu.double()[live], 0.5 * T.tn_products(dy, x, s1, m)[0][live])
        assert torch.equal(T.tn_emulate(dy, x, s1, m, 0.5, 2, 0).double(), 0.5 * T.tn_products(dy, x, s1, m)[0])
    s = T.src_index(1, T.geo_of(1, (1, 10, 12, 3, 1, 12, 12)))
    assert T.mask_of(s) == 0x010                                          # h, w <= dil: the centre tap alone


def test_frame_detects_a_store_outside_the_logical_tensor():
    f = T.Frame((2, 3, 5), (40, 8, 1), BF)
    assert f.host.isnan().all() and f.idx.min() == 16 and f.host.numel() == 16 + 40 + 2 * 8 + 4 + 1 + 72
    f.put(torch.ones(2, 3, 5))
    f.dev = f.host.clone()
    assert torch.equal(f.result().float(), torch.ones(2, 3, 5))
    f.dev[16 + 5] = 0.0                                                   # the padding column behind row 0
    try:
        f.result()
    except AssertionError as e:
        assert "outside the logical tensor" in str(e)
    else:
        raise AssertionError("an over-wide store went unnoticed")


def test_case_tables_reach_every_variant_and_path():
    nt = {}
    for table in (T.NT_PLAIN, T.NT_NARROW, T.NT_ATTN, T.NT_GATHER, T.NT_REGION, T.NT_COLSTATS):
        for name, s in table.items():
            for tk in ("", "64", "32"):
                nt[(name, tk)] = (s, T.nt_spec_variant(s, True, env={"GLF_S16_TK": tk}))
    kernels = {v["kernel"] for _, v in nt.values()}
    assert kernels == {f"s16_rows_kernel<{g}, {bn}, {tk}>" for g in ("true", "false") for bn, tk in ((64, 64), (128, 32), (128, 64))}
    default = {k[0]: v for k, v in nt.items() if k[1] == ""}
    assert {v[1]["tk"] for v in default.values() if v[1]["region"] and v[1]["bn"] == 128} == {64}
    assert any(v["region"] and v["tk"] == 32 for (_, tk), (_, v) in nt.items() if tk == "32")
    assert any(v["kernel"] == "s16_rows_kernel<false, 128, 64>" for (_, tk), (_, v) in nt.items() if tk == "64")
    assert {v["ntiles_max"] for _, v in nt.values()} >= {1, 2, 4}
    for g in (1, 2):
        assert any(s["gather"] == g and v["census"] for s, v in default.values())
        assert any(s["gather"] == g and v["region"] for s, v in default.values())
    slow = [s["conv"] for s, v in default.values() if v["slow_gather"]]
    assert len({c[1] for c in slow}) >= 3                                  # the map_src path at 9 -> 5, 14 -> 7 and 55 -> 28
    assert any(not v["wide"] for _, v in default.values()) and any(v["wide"] for _, v in default.values())
    assert {s["M"] for s in T.NT_PLAIN.values()} == {1, 37, 255, 256, 257, 517, 1100}
    assert {s["N"] for s in T.NT_PLAIN.values()} == {8, 40, 64, 72, 128, 136, 260, 384}
    assert {s["K"] for s in T.NT_PLAIN.values()} == {64, 128, 192, 512, 2048}
    assert {s["batch"] for s in T.NT_PLAIN.values()} == {1, 3} and {s["alpha"] for s in T.NT_PLAIN.values()} == {1.0, 0.5, -2.0}
    assert {s["bias"] for s in T.NT_PLAIN.values()} == {True, False}
    assert all(s["lda"] > s["K"] and s["ldb"] > s["K"] and s["ldc"] > s["N"] for s in T.NT_PLAIN.values())
    assert any(s["colstats"] and v["region"] for s, v in default.values()) and any(s["colstats"] and s["gather"] and not v["region"] for s, v in default.values())
    tn = {k: T.tn_spec_variant(s) for k, s in {**T.TN_PLAIN, **T.TN_GATHER}.items()}
    assert {v["SL"] for v in tn.values()} == {0, 1, 4, 16}
    assert any(v["empty_slices"] > 0 for v in tn.values()) and any(v["k_tail"] for v in tn.values())
    assert {s["K"] for s in T.TN_PLAIN.values()} == {1, 63, 64, 65, 100, 1000, 4099}
    assert {s["M"] for s in T.TN_PLAIN.values()} == {8, 64, 136, 256, 264} and {s["N"] for s in T.TN_PLAIN.values()} == {8, 64, 128, 200}
    assert {s["split"] for s in T.TN_PLAIN.values()} == {1, 2, 3, 7, 16, 40} and {s["batch"] for s in T.TN_PLAIN.values()} == {1, 3}
    assert any(s["rect"] == 1 and s["split"] > 1 for s in T.TN_GATHER.values()) and any(s["mask"] for s in T.TN_GATHER.values())
