"""``ops.linear.issue_wgrad``: the one place that puts a weight gradient on the side stream and keeps its operands
alive until ``join_wgrad``.  A bf16 and an fp8 weight gradient of gw[256, 256] from 256 tokens (the smallest shape
the fp8 kernel takes: tokens % 128 == 0, M, N >= 256), with the overlap on against the overlap off."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import fp8, gemm
from nanodiloco_amd.ops.linear import join_wgrad, wgrad_bf16, wgrad_outstanding

pytestmark = pytest.mark.gpu
TOKENS, M, N = 256, 256, 256


@pytest.fixture(autouse=True)
def _gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    prev = ops.wgrad_overlap_enabled()
    yield
    join_wgrad()
    ops.set_wgrad_overlap(prev)
    ops.set_backend("auto")


def _q8(x, fmt):
    scale = (fp8.FMAX[fmt] / x.abs().amax() / 2).reshape(1).float()
    return fp8.cast(x, scale, fmt), (1.0 / scale).contiguous()


def test_issue_wgrad_side_stream_matches_in_place():
    torch.manual_seed(0)
    dy = torch.randn(TOKENS, M, device="cuda").bfloat16()
    x = torch.randn(TOKENS, N, device="cuda").bfloat16()
    dy8, inv_dy = _q8(dy, fp8.E5M2)
    x8, inv_x = _q8(x, fp8.E4M3)
    gw0 = torch.randn(M, N, device="cuda")
    assert gemm.wgrad_supported(gw0, dy, x) and gemm.wgrad_f8_supported(gw0, dy8, x8)  # the own kernels
    res = {}
    for overlap in (0, 1):
        ops.set_wgrad_overlap(overlap)
        gw, gw8 = gw0.clone(), gw0.clone()
        wgrad_bf16(gw, dy, x)
        fp8.issue_wgrad_f8(gw8, dy8, x8, inv_dy, inv_x)
        pending, keep = wgrad_outstanding()
        if overlap:
            # before the join: both launches are outstanding on this device and their operands are referenced
            assert pending == {torch.cuda.current_device()}
            assert len(keep) == 2 and keep[0][0] is dy and keep[0][1] is x and keep[1][0] is dy8 and keep[1][1] is x8
        else:
            assert not pending and not keep
        join_wgrad()
        assert wgrad_outstanding() == (set(), [])
        torch.cuda.synchronize()
        res[overlap] = (gw, gw8)
    # the same kernels with the same split counts on either stream: bitwise
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][0], gw0) and not torch.equal(res[0][1], gw0)
