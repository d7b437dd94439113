"""Error feedback of the quantised outer transport, PyTorch path (CPU): ``ops.pseudograd_q_ef`` and
``ops.qreduce_ef`` against the in-test oracle of tests/_qef_checks.py; the same checks run on the HIP kernels in
tests/test_qef_gpu.py."""
import pytest
import torch

from nanodiloco_amd import ops

from . import _qef_checks as chk
from . import _qoracle as qo

BITS = [8, 4]
WORKERS = [1, 2, 3, 8]
CHUNKS = (256, 256 * 5)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,w", qo.SIZES)
def test_zero_residual_sends_the_stateless_bytes(n, w, bits):
    chk.check_zero_anchor_stage1(n, w, bits, "cpu")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("w", WORKERS)
def test_zero_residual_reduces_to_the_stateless_bytes(w, bits):
    for c in CHUNKS:
        chk.check_zero_anchor_stage2(c, w, bits, "cpu")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,w", qo.SIZES)
def test_sender_residual_matches_oracle_bitwise(n, w, bits):
    chk.check_nonzero_stage1(n, w, bits, "cpu")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("w", WORKERS)
def test_reducer_residual_matches_oracle_bitwise(w, bits):
    for c in CHUNKS:
        chk.check_nonzero_stage2(c, w, bits, "cpu")


@pytest.mark.parametrize("bits", BITS)
def test_nonfinite_blocks_poison_only_their_own_residuals(bits):
    chk.check_nonfinite_stage1(bits, "cpu")
    chk.check_nonfinite_stage2(bits, "cpu")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("w", [1, 3])
def test_delivered_sum_stays_within_half_a_step_per_stage(w, bits):
    chk.check_delivered_sum(w, bits, "cpu")


def test_argument_checks():
    x, e = torch.zeros(300), torch.zeros(300)
    wire = torch.zeros(2 * 260, dtype=torch.uint8)
    ops.pseudograd_q_ef(x, x, e, wire, 2, 256, 8)
    with pytest.raises(ValueError):  # 300 elements do not fit one chunk of 256
        ops.pseudograd_q_ef(x, x, e, wire[:260], 1, 256, 8)
    with pytest.raises(ValueError):  # wire buffer of the wrong size
        ops.pseudograd_q_ef(x, x, e, wire[:100], 2, 256, 8)
    with pytest.raises(ValueError):  # the residual covers the span, element for element
        ops.pseudograd_q_ef(x, x, torch.zeros(256), wire, 2, 256, 8)
    with pytest.raises(ValueError):
        ops.pseudograd_q_ef(x, x, e.double(), wire, 2, 256, 8)
    out = torch.zeros(260, dtype=torch.uint8)
    ops.qreduce_ef(wire, 2, 256, 8, torch.zeros(256), out)
    with pytest.raises(ValueError):
        ops.qreduce_ef(wire[:260], 2, 256, 8, torch.zeros(256), out)
    with pytest.raises(ValueError):  # one chunk of residual
        ops.qreduce_ef(wire, 2, 256, 8, torch.zeros(512), out)
