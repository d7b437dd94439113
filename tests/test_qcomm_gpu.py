"""HIP kernels of the block-quantised outer transport (csrc/qcomm.hip) against the in-test oracle of
tests/_qoracle.py -- the checks of tests/_qcomm_checks.py on the GPU -- and the one-rank RCCL run of
tests/_qcomm_rccl_check.py in a process of its own.

Multi-rank RCCL cannot run on a one-GPU box (RCCL refuses duplicate devices): the 2/3/4-rank coverage of the
all-to-all + all-gather scheme is the gloo suite of tests/test_qcomm_e2e_cpu.py."""
import os
import subprocess
import sys

import pytest
import torch

from . import _qcomm_checks as chk
from . import _qoracle as qo
from ._mp import child_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = [8, 4]
# 8193 quantisation blocks: one more than the capped grid (2048 workgroups x 4 waves) covers in one pass
WRAP = 8193 * qo.QB
SIZES = qo.SIZES + [(WRAP - 100, 1), (WRAP, 3)]


@pytest.fixture(autouse=True)
def _gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,w", SIZES)
def test_pseudograd_q_exact_inputs_bitwise(n, w, bits):
    chk.check_exact_quantiser(n, w, bits, "cuda")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,w", SIZES)
def test_pseudograd_q_random_inputs_error_bound(n, w, bits):
    chk.check_random_quantiser(n, w, bits, "cuda")


@pytest.mark.parametrize("bits", BITS)
def test_zero_nonfinite_blocks_and_nibble_order(bits):
    chk.check_special_blocks(bits, "cuda")


@pytest.mark.parametrize("bits", BITS)
def test_tiny_amax_block_keeps_zero_codes(bits):
    chk.check_tiny_block(bits, "cuda")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("w", [1, 2, 3, 8])
def test_qreduce_exact_inputs_bitwise(w, bits):
    for c in (256, 256 * 5):
        chk.check_qreduce(c, w, bits, "cuda", exact=True)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("w", [1, 2, 3, 8])
def test_qreduce_random_inputs_error_bound(w, bits):
    for c in (256, 256 * 5):
        chk.check_qreduce(c, w, bits, "cuda", exact=False)


@pytest.mark.parametrize("bits", BITS)
def test_qreduce_grid_stride_wraps(bits):
    chk.check_qreduce(WRAP, 2, bits, "cuda", exact=True)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("shadow", [True, False])
def test_outer_nesterov_q_equals_outer_nesterov_bitwise(bits, first, shadow):
    """master, sync, momentum and the bf16 shadow equal nd_outer_nesterov fed with codes.float() * scale."""
    for n, w in SIZES[:-2]:
        chk.check_outer_q(n, w, bits, "cuda", first, shadow)
        chk.check_outer_q(n, w, bits, "cuda", first, shadow, exact=False)
    chk.check_outer_q(WRAP - 100, 3, bits, "cuda", first, shadow, exact=False)


def test_kernel_launchers_reject_misaligned_buffers():
    from nanodiloco_amd import ops
    x = torch.zeros(1024 + 1, device="cuda")
    out = torch.zeros(4 * 260, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="nd_pseudograd_q"):
        ops.pseudograd_q(x[1:], x[1:], out, 1, 1024, 8)  # fp32 spans must be 16-byte aligned


def test_quantised_outer_step_one_rank_rccl():
    env = child_env(OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "_qcomm_rccl_check.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "QCOMM_RCCL_CHECK_PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
