"""``ops.gemv_w4`` (csrc/gemv_w4.hip) on the MI355X.  (8, 128): one step on one wave, N below a tile; (40, 384): an N
tail, three waves live; (272, 2688): 21 steps, the most in configs/.  The partition keeps K <= 8192 in one slice, so no K
of configs/ reaches the workspace: (272, 8320) is the smallest K that does, in 2 slices of 64 steps and 1."""
import pytest
import torch

from nanodiloco_amd.ops import gemv

from . import _gemm_exact as ge
from . import _oracle64 as o64
from ._frames import assert_frame_intact, framed_flat
from ._model_oracle import spying
from .test_gemv_w8_gpu import _hip  # noqa: F401  (autouse: HIP backend, skip without a GPU)

pytestmark = pytest.mark.gpu
DEV, BF16, REPORT = "cuda", torch.bfloat16, {}
MS, SHAPES = (1, 3, 16), ((8, 128), (40, 384), (272, 2688), (272, 8320))


@pytest.mark.parametrize("block", range(8))
def test_decode_table(block):
    # every byte value four times, every exponent on every channel; row i of x selects k = 16 block + i
    codes = (torch.arange(16 * 64) % 256).to(torch.uint8).view(16, 64).to(DEV)
    exps = torch.tensor([-100, -1, 0, 100], dtype=torch.int8)[(torch.arange(16)[:, None] + torch.arange(4)) % 4].to(DEV)
    x = torch.zeros(16, 128, dtype=BF16, device=DEV)
    x[torch.arange(16), 16 * block + torch.arange(16)] = 1
    want = gemv.dequantize_weight_fp4(codes, exps)[:, 16 * block:16 * block + 16].t().double() + 0.0
    ge.expect_bits(gemv.gemv_w4(x, codes, exps), want, name=f"decode table, block {block}")


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", MS)
def test_exact(M, N, K):
    # x in [-4, 4], codes up to 6, exponents in [-2, 2]: every partial sum is a multiple of 1/8 below 2^24
    assert 8 * ge.exact_bound(K, 4, 6 * 4) < ge.EXACT_LIMIT
    x = ge.int_operand(M, K, -4, 4, BF16, 1, DEV)
    codes = ge.int_operand(N, K // 2, 0, 255, BF16, 2, DEV).to(torch.uint8)  # random nibbles
    exps = ge.int_operand(N, K // 32, -2, 2, BF16, 3, DEV).to(torch.int8)
    big, flat = framed_flat(M * N, BF16)
    out = gemv.gemv_w4(x, codes, exps, out=flat.view(M, N))
    ge.expect_bits(out, ge.exact_nt(x, gemv.dequantize_weight_fp4(codes, exps)), name=f"gemv_w4 {M}x{N}x{K}")
    assert_frame_intact(big, flat)


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", MS)
def test_against_float64(M, N, K):
    torch.manual_seed(M * 1000 + N)
    x = o64.spiked(M, K, DEV).bfloat16()
    # edges on channels of their own: 0 a zero group, 1 a last group of +-6, 2 / 3 every exponent 100 / -100
    codes, exps = gemv.quantize_weight_fp4(torch.randn(N, K, device=DEV) * 0.02)
    codes[0, :16], exps[0, 0], codes[1, K // 2 - 16:], exps[2], exps[3] = 0, 0, 0xf7, 100, -100
    Wd = gemv.dequantize_weight_fp4(codes, exps)
    out = gemv.gemv_w4(x, codes, exps)
    ref, twin = x.double() @ Wd.double().T, x.float() @ Wd.float().T
    for name, cols in (("gemv_w4.exp+100", [2]), ("gemv_w4.exp-100", [3]), ("gemv_w4", [0, 1] + list(range(4, N)))):
        o64.check(out[:, cols], ref[:, cols], twin[:, cols], name=name, report=REPORT, note=f"M {M} N {N} K {K}")
    print(f"[slack] needs margin {REPORT} (allowed {o64.MARGIN})")


@pytest.mark.parametrize("N,K", SHAPES)
def test_row_invariance(N, K):
    torch.manual_seed(N)
    x = o64.spiked(16, K, DEV).bfloat16()
    codes, exps = gemv.quantize_weight_fp4(torch.randn(N, K, device=DEV) * 0.02)
    full = gemv.gemv_w4(x, codes, exps)
    for i in (0, 6, 15):
        one = gemv.gemv_w4(x[i:i + 1], codes, exps)
        three = gemv.gemv_w4(torch.stack([x[(i + 5) % 16], x[(i + 9) % 16], x[i]]), codes, exps)
        assert torch.equal(full[i].view(torch.int16), one[0].view(torch.int16)), (i, "M = 1")
        assert torch.equal(full[i].view(torch.int16), three[2].view(torch.int16)), (i, "M = 3, row 2")


def test_launcher_refusals():
    assert gemv.gemv_w4_workspace_numel(272, 8320) == 2 * 16 * 272 and not gemv.gemv_w4_workspace_numel(272, 8192)
    codes, exps = gemv.quantize_weight_fp4(torch.randn(20, 256, device=DEV))
    x = torch.ones(17, 256, dtype=BF16, device=DEV)
    off = torch.zeros(20 * 128 + 16, dtype=torch.uint8, device=DEV)[1:1 + 20 * 128].view(20, 128)
    with spying() as spy:
        for args in ((x, codes, exps),  # M = 17
                     (x[:2, :96], codes[:, :48].contiguous(), exps[:, :3].contiguous()),  # K = 96
                     (x[:2], off, exps)):  # misaligned codes
            with pytest.raises(ValueError):
                gemv.gemv_w4(*args)
        assert not spy.calls["nd_gemv_w4"]
