"""HIP kernels of the top-k sparse transport (csrc/sparse_comm.hip) against the in-test oracle of
tests/_topk_oracle.py -- the checks of tests/_topk_checks.py on the GPU --, the degenerate equivalence with the
dense transport, and the one-rank RCCL run of tests/_topk_rccl_check.py in a process of its own.

Multi-rank RCCL cannot run on a one-GPU box: the 2/3/4-rank coverage of the all-gather scheme is the gloo suite of
tests/test_topk_e2e_cpu.py."""
import os
import subprocess
import sys

import pytest
import torch

from . import _topk_checks as chk
from ._mp import child_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRAP_CHUNKS = 2048 + 1  # one more chunk than the capped grid has workgroups


@pytest.fixture(autouse=True)
def _gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nanodiloco_amd import ops
    prev = ops.get_backend()
    ops.set_backend("hip")
    yield
    ops.set_backend(prev)


@pytest.mark.parametrize("vdt", chk.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", chk.KS)
@pytest.mark.parametrize("n", chk.SIZES)
def test_select_equals_oracle_bitwise(n, k, vdt):
    for kind in chk.KINDS:
        chk.check_select(n, k, vdt, "cuda", kind)


@pytest.mark.parametrize("vdt", chk.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", chk.KS)
def test_select_grid_stride_wraps(k, vdt):
    chk.check_select_wrap(WRAP_CHUNKS, k, vdt, "cuda")


@pytest.mark.parametrize("vdt", chk.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("w", [1, 2, 3, 8])
def test_apply_equals_nd_outer_nesterov_bitwise(w, vdt):
    for n in chk.SIZES:
        for k in (7, 256):
            for first in (True, False):
                chk.check_apply(n, k, w, vdt, "cuda", first, shadow=first)
                chk.check_apply(n, k, w, vdt, "cuda", first, shadow=not first, seed=1)
    chk.check_apply(chk.SIZES[2], 4096, w, vdt, "cuda", False, shadow=False)
    chk.check_apply(chk.SIZES[2], 1, w, vdt, "cuda", True, shadow=True)


@pytest.mark.parametrize("vdt", chk.DTYPES, ids=["fp32", "bf16"])
def test_apply_grid_stride_wraps(vdt):
    chk.check_apply(WRAP_CHUNKS * 4096 - 100, 7, 2, vdt, "cuda", False, shadow=True)


@pytest.mark.parametrize("vdt", chk.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", [1, 64, 4096])
def test_sent_plus_residual_conserves_the_pseudo_gradient(k, vdt):
    for n in (chk.SIZES[2], 5):
        chk.check_conservation(n, k, vdt, "cuda")


def test_kernel_launchers_reject_misaligned_buffers():
    from nanodiloco_amd import ops
    x = torch.zeros(4096 + 1, device="cuda")
    slot = torch.zeros(ops.topk_slot_bytes(4096, 7, torch.float32), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="nd_pseudograd_topk"):
        ops.pseudograd_topk(x[1:], x[1:], torch.zeros(4096, device="cuda"), slot, 7, torch.float32)
    with pytest.raises(RuntimeError, match="nd_outer_nesterov_topk"):
        ops.outer_nesterov_topk(x[1:], x[1:].clone(), slot, 1, 7, torch.float32, torch.zeros(4096, device="cuda"), None,
                                1.0, 0.7, 0.9, True)


def test_k_4096_fp32_equals_dense_transport_one_worker():
    from nanodiloco_amd.config import LlamaConfig
    from nanodiloco_amd.models import LlamaForCausalLM
    from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
    from nanodiloco_amd.parallel.diloco import Diloco
    from nanodiloco_amd.parallel.dist import DistEnv
    from nanodiloco_amd.parallel.transports import DenseTransport, TopKTransport
    cfg = dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_hidden_layers=2, vocab_size=1000,
               rms_norm_eps=1e-5)
    dev = torch.device("cuda")
    made = []
    for topk in (4096, 0):
        m = LlamaForCausalLM(LlamaConfig(**cfg), dev, torch.bfloat16).init_weights(7)
        dl = Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store, lr=0.7, momentum=0.9), 1, 100, 2,
                    env=DistEnv(device=dev), comm_dtype=torch.float32, topk=topk)
        made += [m, dl]
    assert isinstance(made[1].transport, TopKTransport) and isinstance(made[3].transport, DenseTransport)
    chk.check_degenerate(*made)


def test_topk_outer_step_one_rank_rccl():
    env = child_env(OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "_topk_rccl_check.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "TOPK_RCCL_CHECK_PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
