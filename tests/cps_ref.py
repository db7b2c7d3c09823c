"""Float64 restatement of glf_cps_bce_sum (csrc/pointwise.hip), the cross pseudo supervision loss: helper of
tests/test_cps_ref_cpu.py and tests/test_gpu_cps_loss.py.  A plain module, not a conftest.

Built from pointwise_ref.bce_ref and overlap_ref: each map's hard prediction -- label = x > 0, which is sigmoid(x) > 0.5 wherever
pointwise_ref.overlap_condition holds -- is the other map's target, a constant.  The per-element arithmetic is bce_kernel's and the
two directions meet in double, so K_BCE and K_BCE_DX of pointwise_ref carry over unchanged."""
import torch

from pointwise_ref import K_BCE, K_BCE_DX, TINY, bce_ref, overlap_condition, overlap_ref  # noqa: F401  (re-exported for the tests)

PAIRS_A = [0.0, 0.0, 1.5, -2.5]              # with PAIRS_B: the pairs (0, 0), (0, +), (+, 0), (-, +)
PAIRS_B = [0.0, 2.25, 0.0, 0.75]


def plant_pairs(a, b):
    """overwrite the first min(numel, 4) positions of both (float64 holding fp32 values) with the four sign pairs"""
    k = min(a.numel(), 4)
    a[:k] = torch.tensor(PAIRS_A[:k], dtype=a.dtype)
    b[:k] = torch.tensor(PAIRS_B[:k], dtype=b.dtype)
    return a, b


def cps_ref(a, b, g):
    """(loss, loss_mag, da, da_mag, db, db_mag, stats): loss = sum bce(a, on(b)) + sum bce(b, on(a)); da = (sigmoid(a) - on(b)) g,
    db = (sigmoid(b) - on(a)) g; stats = int64 counts of (on(a), on(b)) = 11, 10, 01, 00 -- overlap_ref(a, on(b))."""
    ta, tb = (a > 0).to(a.dtype), (b > 0).to(b.dtype)
    la, la_mag, da, da_mag = bce_ref(a, tb, g)
    lb, lb_mag, db, db_mag = bce_ref(b, ta, g)
    return la + lb, la_mag + lb_mag, da, da_mag, db, db_mag, overlap_ref(a, tb)
