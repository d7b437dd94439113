"""HIP kernels of the error-feedback transport (csrc/qcomm.hip: nd_pseudograd_q_ef, nd_qreduce_ef) against the
in-test oracle of tests/_qef_checks.py -- the checks of tests/test_qef_cpu.py on the GPU, plus the grid-wrap
sizes -- and the one-rank RCCL run of tests/_qef_rccl_check.py in a process of its own.

As for the stateless transport, the multi-rank coverage of the scheme is the gloo suite
(tests/test_qef_e2e_cpu.py): RCCL refuses duplicate devices on a one-GPU box."""
import os
import subprocess
import sys

import pytest
import torch

from . import _qef_checks as chk
from . import _qoracle as qo
from ._mp import child_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = [8, 4]
WORKERS = [1, 2, 3, 8]
CHUNKS = (256, 256 * 5)
# 8193 quantisation blocks: one more than the capped grid (2048 workgroups x 4 waves) covers in one pass
WRAP = 8193 * qo.QB
SIZES = qo.SIZES + [(WRAP - 100, 1), (WRAP, 3)]


@pytest.fixture(autouse=True)
def _gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,w", SIZES)
def test_zero_residual_sends_the_stateless_bytes(n, w, bits):
    chk.check_zero_anchor_stage1(n, w, bits, "cuda")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("w", WORKERS)
def test_zero_residual_reduces_to_the_stateless_bytes(w, bits):
    for c in CHUNKS:
        chk.check_zero_anchor_stage2(c, w, bits, "cuda")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n,w", SIZES)
def test_sender_residual_matches_oracle_bitwise(n, w, bits):
    chk.check_nonzero_stage1(n, w, bits, "cuda")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("w", WORKERS)
def test_reducer_residual_matches_oracle_bitwise(w, bits):
    for c in CHUNKS:
        chk.check_nonzero_stage2(c, w, bits, "cuda")


@pytest.mark.parametrize("bits", BITS)
def test_reducer_grid_stride_wraps(bits):
    chk.check_zero_anchor_stage2(WRAP, 2, bits, "cuda")
    chk.check_nonzero_stage2(WRAP, 2, bits, "cuda")


@pytest.mark.parametrize("bits", BITS)
def test_nonfinite_blocks_poison_only_their_own_residuals(bits):
    chk.check_nonfinite_stage1(bits, "cuda")
    chk.check_nonfinite_stage2(bits, "cuda")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("w", [1, 3])
def test_delivered_sum_stays_within_half_a_step_per_stage(w, bits):
    chk.check_delivered_sum(w, bits, "cuda")


def test_launchers_reject_a_misaligned_or_missing_residual():
    """hipErrorInvalidValue and no launch: wire and residual keep their sentinels."""
    from nanodiloco_amd import ops
    from nanodiloco_amd.ops import _ext
    n, c = 1024, 1024
    x = torch.ones(n, device="cuda")
    e = torch.full((n + 4,), 3.0, device="cuda")
    wire = torch.full((2 * qo.chunk_bytes(c, 8),), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((qo.chunk_bytes(c, 8),), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="nd_pseudograd_q_ef"):
        ops.pseudograd_q_ef(x, x, e[1:1 + n], wire[:qo.chunk_bytes(c, 8)], 1, c, 8)
    with pytest.raises(RuntimeError, match="nd_qreduce_ef"):
        ops.qreduce_ef(wire, 2, c, 8, e[1:1 + n], out)
    lib, st = _ext.lib(), _ext.stream_ptr(x.device)
    for bits in BITS:
        assert lib.nd_pseudograd_q_ef(_ext.ptr(x), _ext.ptr(x), 0, n, _ext.ptr(wire), 1, c // 256, bits, st) != 0
        assert lib.nd_qreduce_ef(_ext.ptr(wire), 2, c // 256, bits, 0, _ext.ptr(out), st) != 0
    torch.cuda.synchronize()
    assert bool((wire == 0xA5).all()) and bool((out == 0xA5).all()) and bool((e == 3.0).all())


def test_error_feedback_outer_step_one_rank_rccl():
    env = child_env(OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "_qef_rccl_check.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "QEF_RCCL_CHECK_PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
