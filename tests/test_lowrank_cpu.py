"""PyTorch path of the low-rank transport ops (ops/lowrank_comm.py) against the float64 oracle of
tests/_lowrank_oracle.py -- the checks of tests/_lowrank_checks.py on the CPU --, the plan at real model sizes and the
option rules of ``Diloco`` and the command line."""
import json
import os

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.main import parse_args
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.models.param_store import ParamStore
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
from nanodiloco_amd.parallel.diloco import Diloco, _check_options
from nanodiloco_amd.parallel.dist import DistEnv
from nanodiloco_amd.parallel.transports import DenseTransport, LowRankTransport

from . import _lowrank_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(chk.CASES)
TINY = dict(vocab_size=256, hidden_size=128, intermediate_size=320, num_attention_heads=4, num_key_value_heads=2,
            num_hidden_layers=2, max_position_embeddings=64)


@pytest.fixture(autouse=True)
def _no_dist_env():
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)


@pytest.mark.parametrize("case", CASES)
def test_dot_products_within_forward_bound(case):
    print(f"{case}: P error / bound {chk.check_project(case, 'cpu'):.3f}, "
          f"Q_loc error / bound {chk.check_backproject(case, 'cpu'):.3f}")


@pytest.mark.parametrize("case", CASES)
def test_orthonormalize_within_4x_sequential_twin(case):
    err, orth = chk.check_orthonormalize(case, "cpu")
    print(f"{case}: P^ error / (4 x twin) {err:.3f}, orthogonality / (4 x twin) {orth:.3f}")


def test_orthonormalize_zero_and_duplicated_columns():
    chk.check_orthonormalize_edges("cpu")


@pytest.mark.parametrize("w", [1, 2, 3, 8])
@pytest.mark.parametrize("case", CASES)
def test_apply_equals_outer_nesterov_bitwise(case, w):
    for first, shadow in ((True, True), (False, False)):
        print(f"{case} W={w}: s error / bound {chk.check_apply(case, 'cpu', w, first, shadow):.3f}")


def test_dead_and_nonfinite_q_columns_are_reseeded():
    chk.check_reseed_nonfinite("cpu")


@pytest.mark.parametrize("case", CASES)
def test_exact_recovery_of_a_rank_r_pseudo_gradient(case):
    print(f"{case}: |e| / composed bound {chk.check_exact_recovery(case, 'cpu'):.4f}")


@pytest.mark.parametrize("case", CASES)
def test_sent_plus_residual_conserves_the_pseudo_gradient(case):
    print(f"{case}: conservation error / bound {chk.check_conservation(case, 'cpu'):.3f}")


@pytest.mark.parametrize("case", CASES)
def test_zero_step_and_repeatability(case):
    chk.check_zero_step(case, "cpu")
    chk.check_repeatable(case, "cpu")


def test_pytorch_path_refuses_a_bad_table_or_buffer():
    plan, span = chk.make_plan("r8")
    z = torch.zeros(span)
    w1, w2 = ops.lowrank_wire_elems(plan)
    with pytest.raises(ValueError, match="wire buffer 1"):
        ops.lowrank_project(z, z.clone(), z.clone(), torch.zeros(w2), torch.zeros(w1 + 1), plan)
    bad = ops.LowRankPlan.from_layout([(span - 64, 257, 72)], [], 8)
    with pytest.raises(ValueError, match="outside"):
        ops.lowrank_project(z, z.clone(), z.clone(), torch.zeros(bad.wire2_elems), torch.zeros(bad.wire1_elems), bad)
    for r in (0, 33):
        with pytest.raises(ValueError, match="rank"):
            ops.LowRankPlan.from_layout([(0, 256, 256)], [], r)


# ------------------------------------------------------------------------------------------ 9. the plan at real sizes
def _store_layout(config_file):
    """names / shapes / offsets of the model's flat vector; the meta device allocates nothing."""
    cfg = LlamaConfig.from_dict(json.load(open(os.path.join(ROOT, "configs", config_file))))
    groups = []
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        groups.append([p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight"])
        groups.append([p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"])
    return ParamStore(cfg.param_shapes(), "meta", torch.float32, fuse_groups=groups)


@pytest.mark.parametrize("config_file", ["llama_150m.json", "llama_1b.json"])
def test_plan_at_real_sizes(config_file):
    st = _store_layout(config_file)
    line = [f"{config_file}: dense fp32 {4 * st.numel} B"]
    for R in (4, 8, 32):
        plan = ops.LowRankPlan.from_store(st, R)
        w1, w2 = ops.lowrank_wire_elems(plan)
        assert plan._host is None, "a tensor was allocated"
        names = set(plan.mat_names)
        assert "model.embed_tokens.weight" in names and "lm_head.weight" in names
        assert not any("norm" in n for n in names)
        for suffix in ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"):
            assert f"model.layers.0.{'self_attn' if suffix[0] in 'qkvo' else 'mlp'}.{suffix}.weight" in names
        p_spans, q_spans = [], []
        for (off, m, n, po, qo), name in zip(plan.mats, plan.mat_names):
            assert (m, n) == tuple(st.shapes[name]) and off == st.offsets[name]
            assert 0 <= off and off + m * n <= st.numel and off % 4 == 0 and n % 4 == 0 and min(m, n) >= 4 * R
            p_spans.append((po, po + m * R))
            q_spans.append((qo, qo + n * R))
        # [dense | all P] and [all Q]: disjoint, in order, nothing left over
        assert p_spans[0][0] == plan.dense_total and p_spans[-1][1] == w1 and q_spans[0][0] == 0 and q_spans[-1][1] == w2
        for spans in (p_spans, q_spans):
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert plan.dense_total == sum(b - a for a, b in plan.dense) and all(0 <= a < b <= st.numel for a, b in plan.dense)
        assert plan.compressed_elems + plan.dense_total == st.num_params
        table, _ = plan.host_tables()
        assert table.dtype == torch.int64 and table.numel() == 5 * len(plan)
        if config_file == "llama_1b.json":
            # 1.1e9 elements: the element offsets stay below 2^31, the BYTE offsets the kernels form from them do not
            assert 4 * int(table.view(-1, 5)[:, 0].max()) > 2 ** 31 and 4 * st.numel > 2 ** 32
        line.append(f"R={R}: {4 * (w1 + w2)} B ({st.numel / (w1 + w2):.1f}x)")
    print(", ".join(line))


# ------------------------------------------------------------------------------------------ 8. rules
def _mk(lowrank=4, comm=torch.float32, cfg=TINY, **kw):
    m = LlamaForCausalLM(LlamaConfig(**cfg)).init_weights(7)
    dl = Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store, lr=0.7, momentum=0.9), 2, 8, 4,
                env=kw.pop("env", None) or DistEnv(device=torch.device("cpu")), comm_dtype=comm, lowrank=lowrank, **kw)
    return m, dl


def test_rules_through_diloco():
    for r in (-1, 33):
        with pytest.raises(ValueError, match="lowrank"):
            _mk(r)
    for comm in (torch.bfloat16, "int8", "int4"):
        with pytest.raises(ValueError, match="fp32 factors"):
            _mk(comm=comm)
    with pytest.raises(ValueError, match="error_feedback"):
        _mk(error_feedback=True)
    with pytest.raises(ValueError, match="topk"):
        _mk(topk=7)
    with pytest.raises(ValueError, match="overlap"):
        _mk(overlap=True)
    with pytest.raises(ValueError, match="fragments"):
        _mk(fragments=1, stream_overlap=0)
    with pytest.raises(ValueError, match="inner_dp"):
        _check_options(True, torch.float32, inner_dp=2, lowrank=4)
    with pytest.raises(ValueError, match="nothing to compress"):
        _mk(32, cfg=dict(TINY, hidden_size=64, intermediate_size=96, vocab_size=100))  # min(m, n) < 128 everywhere
    net = torch.nn.Linear(4, 4)
    with pytest.raises(ValueError, match="ModuleDiloco"):
        Diloco(net, torch.optim.AdamW(net.parameters(), lr=1e-3), torch.optim.SGD(net.parameters(), lr=0.7), 0, 10,
               lowrank=4)
    assert _check_options(True, torch.float32, lowrank=1) == 0 and _check_options(True, torch.float32, lowrank=32) == 0
    # off by default: the dense transport, and no low-rank state anywhere
    _, dl = _mk(0)
    assert isinstance(dl.transport, DenseTransport) and not hasattr(dl, "lowrank_residual")
    assert dl.transport.shared_tensors() == {} and "comm_lowrank" not in dl.transport.shared_state()[0]
    m, dl = _mk(8)
    assert isinstance(dl.transport, LowRankTransport) and not bool(dl.lowrank_residual.any())
    assert torch.equal(dl.lowrank_q, dl.transport.plan.init_q())
    assert dl.transport.shared_state()[0]["comm_lowrank"]["rank"] == 8 and set(dl.transport.shared_tensors()) == {"lowrank.q"}
    # one worker: no traffic is counted, as for every transport
    assert dl.bytes_per_outer_step == 0 and dl.transport.bytes_per_step == 4 * sum(ops.lowrank_wire_elems(dl.transport.plan))


def test_rules_through_the_cli():
    from nanodiloco_amd.trainer import Trainer
    assert parse_args([]).comm_rank == 0 and parse_args(["--comm-rank", "8"]).comm_rank == 8
    base = ["--total-steps", "8", "--inner-steps", "4", "--device", "cpu", "--wandb", "off", "--comm-rank", "4"]
    for extra, word in ((["--comm-dtype", "bf16"], "--comm-dtype bf16"), (["--comm-dtype", "int8"], "--comm-dtype int8"),
                        (["--comm-error-feedback", "--comm-dtype", "int8"], "--comm-dtype int8"),
                        (["--comm-error-feedback"], "--comm-error-feedback"), (["--comm-topk", "64"], "--comm-topk"),
                        (["--overlap-outer"], "--overlap-outer"), (["--streaming-fragments", "1"], "--streaming-fragments"),
                        (["--inner-dp", "2"], "--inner-dp"), (["--comm-rank", "33"], "32")):
        with pytest.raises(ValueError, match="--comm-rank") as err:
            Trainer(parse_args(base + extra))
        assert word in str(err.value)


# ------------------------------------------------------------------------------------------ 10. one worker
def test_one_worker_two_outer_steps_against_a_dense_twin():
    chk.check_diloco_one_worker(torch.device("cpu"), torch.float32)
