"""CPU: tests/cps_ref.cps_ref, the float64 restatement that gates glf_cps_bce_sum, against torch autograd of the loss spelled with
F.binary_cross_entropy_with_logits on detached hard labels."""
import pytest
import torch
import torch.nn.functional as F

import cps_ref as CR
import pointwise_ref as R


def _inputs(numel):
    a, b = R.bce_inputs(numel, seed=601)[0], R.bce_inputs(numel, seed=641)[0]
    return CR.plant_pairs(a, b)


@pytest.mark.parametrize("numel", R.BCE_NUMEL + [4099])
@pytest.mark.parametrize("g", [1.0, 1.0 / 256, -0.37])
def test_cps_ref_is_torch_autograd_of_the_two_bce_sums(numel, g):
    a, b = _inputs(numel)
    assert R.overlap_condition(a) and R.overlap_condition(b)
    ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    want = (F.binary_cross_entropy_with_logits(ta, (tb > 0).double(), reduction="sum")
            + F.binary_cross_entropy_with_logits(tb, (ta > 0).double(), reduction="sum"))
    (g * want).backward()
    loss, mag, da, dam, db, dbm, stats = CR.cps_ref(a, b, g)
    assert abs(float(loss) - float(want.detach())) <= 1e-12 * float(mag)
    assert float(mag) >= abs(float(loss))
    assert torch.allclose(da, ta.grad, rtol=0, atol=1e-14 * abs(g)) and torch.allclose(db, tb.grad, rtol=0, atol=1e-14 * abs(g))
    assert bool((dam >= da.abs()).all()) and bool((dbm >= db.abs()).all())
    pa, pb = a > 0, b > 0
    assert stats.dtype == torch.int64 and int(stats.sum()) == numel
    assert stats.tolist() == [int((pa & pb).sum()), int((pa & ~pb).sum()), int((~pa & pb).sum()), int((~pa & ~pb).sum())]
    assert torch.equal(stats, R.overlap_ref(a, pb.double()))


def test_planted_pairs_cover_the_four_sign_cases_and_zero_is_off():
    a, b = _inputs(257)
    assert [(float(x), float(y)) for x, y in zip(a[:4], b[:4])] == list(zip(CR.PAIRS_A, CR.PAIRS_B))
    # a logit of exactly 0 predicts "off": sigmoid(0) = 0.5 is not > 0.5
    _, _, da, _, db, _, stats = CR.cps_ref(a[:4].clone(), b[:4].clone(), 1.0)
    assert stats.tolist() == [0, 1, 2, 1]
    assert float(da[0]) == 0.5 and float(db[0]) == 0.5 and float(da[1]) == -0.5 and float(db[2]) == -0.5
