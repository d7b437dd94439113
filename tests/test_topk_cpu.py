"""The PyTorch path of the top-k sparse transport ops (nanodiloco_amd/ops/sparse_comm.py) against the in-test oracle
of tests/_topk_oracle.py: the checks of tests/_topk_checks.py on CPU.  tests/test_topk_gpu.py runs the same checks
on the HIP kernels."""
import numpy as np
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import sparse_comm

from . import _topk_checks as chk
from . import _topk_oracle as to


@pytest.mark.parametrize("vdt", chk.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", chk.KS)
@pytest.mark.parametrize("n", chk.SIZES)
def test_select_equals_oracle_bitwise(n, k, vdt):
    for kind in chk.KINDS:
        chk.check_select(n, k, vdt, "cpu", kind)


@pytest.mark.parametrize("vdt", chk.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("w", [1, 2, 3, 8])
def test_apply_equals_outer_nesterov_bitwise(w, vdt):
    for n in chk.SIZES:
        for k in (7, 256):
            for first in (True, False):
                chk.check_apply(n, k, w, vdt, "cpu", first, shadow=first)
    chk.check_apply(chk.SIZES[2], 4096, w, vdt, "cpu", False, shadow=False)
    chk.check_apply(chk.SIZES[2], 1, w, vdt, "cpu", True, shadow=True)


@pytest.mark.parametrize("vdt", chk.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", [1, 64, 4096])
def test_sent_plus_residual_conserves_the_pseudo_gradient(k, vdt):
    for n in (chk.SIZES[2], 5):
        chk.check_conservation(n, k, vdt, "cpu")


def test_slot_geometry_and_argument_checks():
    assert sparse_comm.CHUNK == 4096
    for n, k, vdt in ((5, 1, torch.float32), (4096, 7, torch.bfloat16), (3 * 4096 + 5, 64, torch.bfloat16)):
        b = ops.topk_slot_bytes(n, k, vdt)
        assert b == to.slot_bytes(n, k, vdt == torch.bfloat16) and b % 16 == 0
    assert ops.topk_slot_bytes(4096, 64, torch.bfloat16) == 128 + 128
    assert ops.topk_slot_bytes(5, 1, torch.float32) == 16 + 16
    x = torch.zeros(4096)
    slot = torch.zeros(ops.topk_slot_bytes(4096, 7, torch.float32), dtype=torch.uint8)
    for k in (0, 4097):
        with pytest.raises(ValueError, match="k"):
            ops.topk_slot_bytes(4096, k, torch.float32)
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        ops.topk_slot_bytes(4096, 7, torch.float16)
    with pytest.raises(ValueError, match="slot"):
        ops.pseudograd_topk(x, x, x.clone(), slot[:-16], 7, torch.float32)
    with pytest.raises(ValueError, match="residual"):
        ops.pseudograd_topk(x, x, x[:-1].clone(), slot, 7, torch.float32)
    with pytest.raises(ValueError, match="sizes"):
        ops.outer_nesterov_topk(x, x.clone(), slot, 2, 7, torch.float32, x.clone(), None, 0.5, 0.7, 0.9, True)


def test_oracle_bf16_rounding_is_round_to_nearest_even():
    """The oracle's integer bf16 rounding against torch's, on ties, both neighbours of ties, and denormals."""
    bits = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x00008000, 0x00018000, 0x7F7FFFFF, 0x80008000,
                     0x3F800000, 0xBF80C000], dtype=np.uint32)
    got = to.bf16_bits(bits.view(np.float32))
    want = torch.from_numpy(bits.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    assert got[0] == 0x3F80 and got[1] == 0x3F82  # ties go to the even neighbour
