"""Block-quantised outer transport, PyTorch path (CPU): quantiser, reducer and quantised outer update
against the in-test oracle of tests/_qoracle.py; the same checks run on the HIP kernels in
tests/test_qcomm_gpu.py."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import qcomm

from . import _qcomm_checks as chk
from . import _qoracle as qo

BITS = [8, 4]


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,w", qo.SIZES)
def test_quantiser_exact_inputs_bitwise(n, w, bits):
    chk.check_exact_quantiser(n, w, bits, "cpu")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,w", qo.SIZES)
def test_quantiser_random_inputs_error_bound(n, w, bits):
    chk.check_random_quantiser(n, w, bits, "cpu")


@pytest.mark.parametrize("bits", BITS)
def test_zero_nonfinite_blocks_and_nibble_order(bits):
    chk.check_special_blocks(bits, "cpu")


@pytest.mark.parametrize("bits", BITS)
def test_tiny_amax_block_keeps_zero_codes(bits):
    chk.check_tiny_block(bits, "cpu")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("w", [1, 2, 3, 8])
@pytest.mark.parametrize("exact", [True, False])
def test_qreduce_matches_oracle(w, bits, exact):
    for c in (256, 256 * 5):
        chk.check_qreduce(c, w, bits, "cpu", exact)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("first", [True, False])
def test_outer_nesterov_q_equals_fp32_update_on_dequantised(bits, first):
    for n, w in qo.SIZES:
        chk.check_outer_q(n, w, bits, "cpu", first, shadow=True)
        chk.check_outer_q(n, w, bits, "cpu", first, shadow=False, exact=False)


def test_wire_geometry_and_argument_checks():
    assert qcomm.chunk_elems(64, 1) == 256 and qcomm.chunk_elems(700, 3) == 256 and qcomm.chunk_elems(2368, 3) == 1024
    assert qcomm.chunk_bytes(256, 8) == 260 and qcomm.chunk_bytes(256, 4) == 132 and qcomm.chunk_bytes(1024, 8) == 1040
    for c, bits in ((256, 8), (256, 4), (768, 4)):
        assert qcomm.chunk_bytes(c, bits) == qo.chunk_bytes(c, bits) and qcomm.chunk_bytes(c, bits) % 4 == 0
    with pytest.raises(ValueError):
        qcomm.chunk_bytes(200, 8)
    with pytest.raises(ValueError):
        qcomm.chunk_bytes(256, 2)
    x = torch.zeros(300)
    with pytest.raises(ValueError):  # 300 elements do not fit one chunk of 256
        ops.pseudograd_q(x, x, torch.zeros(260, dtype=torch.uint8), 1, 256, 8)
    with pytest.raises(ValueError):  # wire buffer of the wrong size
        ops.pseudograd_q(x, x, torch.zeros(100, dtype=torch.uint8), 2, 256, 8)
    with pytest.raises(ValueError):
        ops.qreduce(torch.zeros(260, dtype=torch.uint8), 2, 256, 8, torch.zeros(260, dtype=torch.uint8))
