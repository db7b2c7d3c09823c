"""glf_split_f16_packed_colsum: the packed pre-split image of glf_split_f16_packed (bit for bit) plus the column sums of its fp32
input from the same pass.  The sums against float64 on the CPU: relative L2 error <= 1.5 x glf_colsum's + 1e-7 (the yardstick of
test_gpu_aspp_centre.py), both printed.  Shapes: fewer rows than a workgroup covers in one pass and several ragged slices x two
float4 columns, two ragged column blocks of 16, twelve blocks of 64 (the stacked projection's width); dense and padded rows."""
import pytest
import torch

from glfusion_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT = -12345.5
GUARD = 64


def _run(x, am, rows, cols, ld):
    pk = torch.full((rows * ld + GUARD,), SENT, device=DEV)
    sums = torch.full((cols + GUARD,), SENT, device=DEV)
    ws = torch.empty(int(lib.glf_bn_workspace(rows, cols)), dtype=torch.float64, device=DEV)
    rc = lib.glf_split_f16_packed_colsum(x.data_ptr(), rows, cols, ld, am.data_ptr(), pk.data_ptr(), ld, sums.data_ptr(), ws.data_ptr(), None)
    assert rc == 0, lib.glf_last_error()
    torch.cuda.synchronize()
    return pk, sums


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("cols", [8, 72, 3072])
@pytest.mark.parametrize("rows", [5, 1031])
def test_image_bits_sums_and_guards(rows, cols, pad):
    ld = cols + pad
    g = torch.Generator().manual_seed(7 * rows + cols + pad)
    x = torch.full((rows, ld), SENT)                     # the padding columns must be neither read into the sums nor written
    x[:, :cols] = torch.randn(rows, cols, generator=g) * 3.0 + 0.5
    ref = x[:, :cols].double().sum(0)
    x = x.to(DEV)
    am = x[:, :cols].abs().max().reshape(1).contiguous()
    pk, sums = _run(x, am, rows, cols, ld)
    pk2, sums2 = _run(x, am, rows, cols, ld)
    want = torch.full((rows * ld,), SENT, device=DEV)
    assert lib.glf_split_f16_packed(x.data_ptr(), rows, cols, ld, am.data_ptr(), want.data_ptr(), ld, None) == 0
    old = torch.empty(cols, device=DEV)
    xs = x[:, :cols].contiguous()
    ws = torch.empty(int(lib.glf_bn_workspace(rows, cols)), dtype=torch.float64, device=DEV)
    assert lib.glf_colsum(xs.data_ptr(), cols, old.data_ptr(), rows, cols, ws.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(pk[:rows * ld].view(torch.int32), want.view(torch.int32)), "the image differs from glf_split_f16_packed's"
    assert bool((pk[rows * ld:] == SENT).all()) and bool((sums[cols:] == SENT).all()), "a write landed behind an output buffer"
    if pad:
        assert bool((pk[:rows * ld].view(rows, ld)[:, cols:] == SENT).all()), "a padding column was written"
    assert torch.equal(pk.view(torch.int32), pk2.view(torch.int32)) and torch.equal(sums.view(torch.int32), sums2.view(torch.int32))
    e_new = float((sums[:cols].cpu().double() - ref).norm() / ref.norm())
    e_old = float((old.cpu().double() - ref).norm() / ref.norm())
    print(f"rows {rows} cols {cols} ld {ld}: split+colsum {e_new:.3e} glf_colsum {e_old:.3e}")
    assert e_new <= 1.5 * e_old + 1e-7, (e_new, e_old)


def test_refusals():
    x = torch.zeros(5 * 16, device=DEV)
    o, s, am = torch.zeros_like(x), torch.zeros(16, device=DEV), torch.ones(1, device=DEV)
    ws = torch.empty(int(lib.glf_bn_workspace(5, 16)), dtype=torch.float64, device=DEV)
    assert lib.glf_split_f16_packed_colsum(x.data_ptr(), 5, 14, 16, am.data_ptr(), o.data_ptr(), 16, s.data_ptr(), ws.data_ptr(), None) != 0
    assert lib.glf_split_f16_packed_colsum(x.data_ptr(), 5, 16, 14, am.data_ptr(), o.data_ptr(), 16, s.data_ptr(), ws.data_ptr(), None) != 0
    assert lib.glf_split_f16_packed_colsum(x.data_ptr(), 5, 16, 16, am.data_ptr(), x.data_ptr(), 16, s.data_ptr(), ws.data_ptr(), None) != 0
    assert lib.glf_split_f16_packed_colsum(None, 5, 16, 16, am.data_ptr(), o.data_ptr(), 16, s.data_ptr(), ws.data_ptr(), None) != 0
