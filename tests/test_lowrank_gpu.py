"""HIP kernels of the low-rank transport (csrc/lowrank_comm.hip) against the float64 oracle of
tests/_lowrank_oracle.py -- the checks of tests/_lowrank_checks.py on the GPU --, the launchers' refusals, one worker
through ``Diloco`` next to a dense twin, and the one-rank RCCL run of tests/_lowrank_rccl_check.py in a process of its
own.

Multi-rank RCCL cannot run on a one-GPU box: the 2- and 3-worker coverage is the gloo suite of
tests/test_lowrank_e2e_cpu.py."""
import os
import subprocess
import sys

import pytest
import torch

from . import _lowrank_checks as chk
from ._mp import child_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(chk.CASES)


@pytest.fixture(autouse=True)
def _gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nanodiloco_amd import ops
    prev = ops.get_backend()
    ops.set_backend("hip")
    yield
    ops.set_backend(prev)


@pytest.mark.parametrize("case", CASES)
def test_dot_products_within_forward_bound(case):
    print(f"{case}: P error / bound {chk.check_project(case, 'cuda'):.3f}, "
          f"Q_loc error / bound {chk.check_backproject(case, 'cuda'):.3f}")


@pytest.mark.parametrize("case", CASES)
def test_orthonormalize_within_4x_sequential_twin(case):
    err, orth = chk.check_orthonormalize(case, "cuda")
    print(f"{case}: P^ error / (4 x twin) {err:.3f}, orthogonality / (4 x twin) {orth:.3f}")


def test_orthonormalize_zero_and_duplicated_columns():
    chk.check_orthonormalize_edges("cuda")


@pytest.mark.parametrize("w", [1, 2, 3, 8])
@pytest.mark.parametrize("case", CASES)
def test_apply_equals_nd_outer_nesterov_bitwise(case, w):
    for first, shadow in ((True, True), (False, False), (False, True)):
        print(f"{case} W={w}: s error / bound {chk.check_apply(case, 'cuda', w, first, shadow):.3f}")


def test_dead_and_nonfinite_q_columns_are_reseeded():
    chk.check_reseed_nonfinite("cuda")


@pytest.mark.parametrize("case", CASES)
def test_exact_recovery_of_a_rank_r_pseudo_gradient(case):
    print(f"{case}: |e| / composed bound {chk.check_exact_recovery(case, 'cuda'):.4f}")


@pytest.mark.parametrize("case", CASES)
def test_sent_plus_residual_conserves_the_pseudo_gradient(case):
    print(f"{case}: conservation error / bound {chk.check_conservation(case, 'cuda'):.3f}")


@pytest.mark.parametrize("case", CASES)
def test_zero_step_and_repeatability(case):
    chk.check_zero_step(case, "cuda")
    chk.check_repeatable(case, "cuda")


def _call(op, plan, t):
    from nanodiloco_amd import ops
    if op == "nd_lowrank_project":
        ops.lowrank_project(t["sync"], t["master"], t["resid"], t["q"], t["wire1"], plan)
    elif op == "nd_lowrank_orthonormalize":
        ops.lowrank_orthonormalize(t["wire1"], plan)
    elif op == "nd_lowrank_backproject":
        ops.lowrank_backproject(t["resid"], t["wire1"], t["wire2"], plan)
    else:
        ops.outer_nesterov_lowrank(t["master"], t["sync"], t["resid"], t["wire1"], t["wire2"], t["q"], t["q0"], t["mom"],
                                   None, plan, 1.0, 0.7, 0.9, True, None)


LAUNCHERS = {"nd_lowrank_project": "sync", "nd_lowrank_orthonormalize": "wire1", "nd_lowrank_backproject": "wire2",
             "nd_outer_nesterov_lowrank": "mom"}


@pytest.mark.parametrize("op", list(LAUNCHERS))
def test_kernel_launchers_reject_misaligned_buffers_and_bad_rows(op):
    """Nothing is launched on a refused call: every buffer keeps its bytes."""
    from nanodiloco_amd import ops
    good, span = chk.make_plan("r8")
    w1, w2 = ops.lowrank_wire_elems(good)

    def buffers(extra=0):
        sizes = dict(sync=span, master=span, resid=span, mom=span, q=w2, q0=w2, wire1=w1, wire2=w2)
        return {k: torch.full((n + extra,), 3.0, device="cuda") for k, n in sizes.items()}

    t = buffers(extra=1)
    views = {k: (v[1:] if k == LAUNCHERS[op] else v[:-1]) for k, v in t.items()}  # one buffer 4 bytes off
    with pytest.raises(RuntimeError, match=op):
        _call(op, good, views)
    (o0, m0, n0), (o1, m1, n1) = [(o, m, n) for o, m, n, _, _ in good.mats]
    rows = {"past the span": [(o0, m0, n0), (span - 64, m1, n1)], "negative": [(-64, m0, n0), (o1, m1, n1)]}
    for why, mats in rows.items():
        bad = ops.LowRankPlan.from_layout(mats, good.dense, 8)
        assert ops.lowrank_wire_elems(bad) == (w1, w2)
        if op == "nd_lowrank_orthonormalize":  # it reads only P: a row whose P lies outside wire 1
            bad.mats[1] = bad.mats[1][:3] + (w1 - 8, bad.mats[1][4])
        t = buffers()
        with pytest.raises(RuntimeError, match=op):
            _call(op, bad, t)
        torch.cuda.synchronize()
        assert all(bool((v == 3.0).all()) for v in t.values()), why
    for r in (0, 33):  # R outside 1 .. 32 never reaches a kernel either
        with pytest.raises(ValueError, match="rank"):
            ops.LowRankPlan.from_layout(good.mats, good.dense, r)


def test_one_worker_two_outer_steps_against_a_dense_twin():
    chk.check_diloco_one_worker(torch.device("cuda"), torch.bfloat16)


def test_lowrank_outer_step_one_rank_rccl():
    env = child_env(OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "_lowrank_rccl_check.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "LOWRANK_RCCL_CHECK_PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
