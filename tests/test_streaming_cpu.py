"""Streaming DiLoCo on CPU/gloo: fragment plan, schedule, validation, the anchor to the classic outer step
(P=1, tau=0, alpha=0 is bitwise ``Diloco.outer_step``), per-fragment golden values, the tau / alpha merge, the
byte accounting, and the CLI with checkpoint / resume."""
import json
import os
import subprocess
import sys

import pytest
import torch

from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
from nanodiloco_amd.parallel.diloco import Diloco
from nanodiloco_amd.parallel.dist import init_distributed
from nanodiloco_amd.parallel.fragments import fragment_due, plan_fragments

from . import _outer_chains as oc
from ._mp import child_env, free_port, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY4 = dict(hidden_size=32, intermediate_size=64, num_attention_heads=2, num_hidden_layers=4, vocab_size=50,
             rms_norm_eps=1e-5)
H = 8


def _model(seed=3):
    return LlamaForCausalLM(LlamaConfig.from_dict(TINY4)).init_weights(seed)


def _diloco(m, env=None, **kw):
    return Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store, lr=0.7, momentum=0.9), 2, 4 * H, H,
                  env=env, **kw)


def _no_group():
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)


# ------------------------------------------------------------------ 1. plan
def _layer_span(st, i):
    first = lambda j: st.offsets[f"model.layers.{j}.self_attn.q_proj.weight"]  # noqa: E731
    return first(i), (first(i + 1) if i + 1 < 4 else st.offsets["model.norm.weight"])


def _covers(spans, a, b):
    return any(x <= a and b <= y for x, y in spans)


@pytest.mark.parametrize("pattern,members", [("strided", [{0, 2}, {1, 3}]), ("sequential", [{0, 1}, {2, 3}])])
def test_plan_two_fragments(pattern, members):
    st = _model().store
    plan = plan_fragments(st, 4, 2, pattern)
    assert len(plan) == 2
    for p, layers in enumerate(members):
        for i in range(4):
            assert _covers(plan[p], *_layer_span(st, i)) == (i in layers), (pattern, p, i)
    assert _covers(plan[0], *st.range("model.embed_tokens.weight"))      # with layer 0
    assert _covers(plan[1], *st.range("model.norm.weight"))              # with layer 3
    assert _covers(plan[1], *st.range("lm_head.weight"))
    assert plan[1][-1][1] == st.numel                                    # trailing padding
    spans = sorted(s for f in plan for s in f)
    assert all(a % 64 == 0 and b % 64 == 0 and a < b for a, b in spans)
    assert spans[0][0] == 0 and spans[-1][1] == st.numel
    assert all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))  # disjoint, no hole
    for f in plan:  # adjacent spans of one fragment are merged
        assert all(f[i][1] < f[i + 1][0] for i in range(len(f) - 1))


def test_plan_one_fragment_is_everything():
    st = _model().store
    assert plan_fragments(st, 4, 1, "strided") == [[(0, st.numel)]]
    assert plan_fragments(st, 4, 1, "sequential") == [[(0, st.numel)]]
    with pytest.raises(ValueError):
        plan_fragments(st, 4, 5, "strided")
    with pytest.raises(ValueError):
        plan_fragments(st, 4, 2, "zigzag")


# ------------------------------------------------------------------ 2. schedule and validation
def test_schedule_h8_p4_tau1():
    _no_group()
    assert [fragment_due(t, 8, 4) for t in range(1, 9)] == [None, 0, None, 1, None, 2, None, 3]
    dl = _diloco(_model(), fragments=4, stream_overlap=1)
    sends, applies = [], []
    for t in range(1, 26):
        ev = dl.stream_step(t)
        if ev and ev["sent"] is not None:
            sends.append((t, ev["sent"]))
        if ev and ev["applied"] is not None:
            applies.append((t, ev["applied"]))
    assert sends == [(2 * k, (k - 1) % 4) for k in range(1, 13)]                 # 2, 4, 6, 8, period 8
    assert applies == [(2 * k + 1, (k - 1) % 4) for k in range(1, 13)]           # 3, 5, 7, 9
    assert dl.outer_step_count == 3 and dl.outer_optimizer.step_count == 3       # one per completed round
    assert dl.fragment_sync_count == 12 and dl.frag_steps == [3, 3, 3, 3]


@pytest.mark.parametrize("kw", [
    dict(fragments=5),                                   # P > L
    dict(fragments=-1),
    dict(fragments=2, stream_overlap=4),                 # tau >= H // P
    dict(fragments=4, stream_overlap=2),
    dict(fragments=2, stream_overlap=-1),
    dict(fragments=2, stream_alpha=-0.1),
    dict(fragments=2, stream_alpha=1.5),
    dict(fragments=2, fragment_pattern="zigzag"),
    dict(fragments=2, overlap=True),
    dict(fragments=2, comm_dtype="int8"),
    dict(fragments=2, comm_dtype="int4"),
    dict(fragments=2, offload_snapshot=True),
])
def test_refused_options(kw):
    _no_group()
    with pytest.raises(ValueError):
        _diloco(_model(), **kw)


def test_refused_more_fragments_than_inner_steps():
    _no_group()
    m = _model()
    with pytest.raises(ValueError):  # P <= H
        Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store), 2, 8, 2, fragments=4)


def test_refused_module_diloco():
    lin = torch.nn.Linear(4, 4)
    with pytest.raises(ValueError, match="ModuleDiloco"):
        Diloco(lin, torch.optim.AdamW(lin.parameters()), torch.optim.SGD(lin.parameters(), lr=0.7), 2, 8, 4,
               fragments=2)


def _refuse_inner_dp(rank, world):
    env = init_distributed("gloo", inner_dp=2)
    with pytest.raises(ValueError, match="inner_dp"):
        _diloco(_model(), env=env, fragments=2)
    return True


def test_refused_inner_dp():
    assert all(run_ranks(_refuse_inner_dp, 2))


def test_outer_step_refused_in_streaming_mode():
    _no_group()
    dl = _diloco(_model(), fragments=2)
    with pytest.raises(RuntimeError):
        dl.outer_step()


# ------------------------------------------------------------------ 3. anchor: P=1, tau=0, alpha=0 == classic
def _anchor(rank, world):
    env = init_distributed("gloo")
    ma, mb = _model(7), _model(7)
    classic, stream = _diloco(ma, env=env), _diloco(mb, env=env, fragments=1)
    g = torch.Generator().manual_seed(100 + rank)
    for k in range(1, 4):
        drift = 0.01 * torch.randn(ma.store.numel, generator=g)
        ma.store.master.add_(drift)
        mb.store.master.add_(drift)
        classic.outer_step()
        ev = stream.stream_step(k * H)
        assert ev == {"sent": 0, "applied": 0}
        assert torch.equal(ma.store.master, mb.store.master)
        assert torch.equal(classic.sync, stream.sync)
        assert torch.equal(classic.outer_optimizer.momentum_buffer, stream.outer_optimizer.momentum_buffer)
    assert stream.outer_step_count == classic.outer_step_count == 3
    assert stream.outer_optimizer.step_count == 3
    return True


def test_one_fragment_is_bitwise_the_classic_outer_step():
    assert all(run_ranks(_anchor, 2))


# ------------------------------------------------------------------ 4. per-fragment golden values
_golden = oc.stream_golden  # shared with tests/test_transports_multiworker_gpu.py


def test_golden_values_per_fragment():
    assert all(run_ranks(_golden, 2))


# ------------------------------------------------------------------ 5. tau and alpha
_tau_alpha = oc.stream_tau_alpha  # shared with tests/test_transports_multiworker_gpu.py


@pytest.mark.parametrize("alpha", [0.5, 0.0])
def test_overlap_window_and_mixing(alpha):
    assert all(run_ranks(_tau_alpha, 2, alpha))


# ------------------------------------------------------------------ 6. bytes
def _bytes(rank, world, comm):
    env = init_distributed("gloo")
    m = _model(5)
    dl = _diloco(m, env=env, fragments=2, comm_dtype=comm)
    size = torch.tensor([], dtype=comm).element_size()
    assert dl.bytes_per_outer_step == 0 and dl.delta.numel() == max(t.total for t in dl.frag_tables)
    seen = []
    for t in range(1, H + 1):
        ev = dl.stream_step(t)
        if ev:
            n = sum(b - a for a, b in dl.frag_tables[ev["sent"]].spans)
            assert dl.bytes_per_outer_step == n * size
            assert dl.buckets_per_outer_step == 1
            seen.append(dl.bytes_per_outer_step)
    assert len(seen) == 2 and sum(seen) == m.store.numel * size
    return True


@pytest.mark.parametrize("comm", [torch.float32, torch.bfloat16])
def test_bytes_per_fragment(comm):
    assert all(run_ranks(_bytes, 2, comm))


def test_span_table_validation():
    from nanodiloco_amd import ops
    x = torch.zeros(512)
    out = torch.zeros(512)
    for bad in ([(0, 100)], [(32, 96)], [(0, 128), (64, 192)], [(128, 192), (0, 64)], [(64, 64)], []):
        with pytest.raises(ValueError):
            ops.frag_pseudograd(x, x, bad, out)
    with pytest.raises(ValueError):  # past the end of the flat buffers
        ops.frag_pseudograd(x, x, [(448, 576)], out)
    with pytest.raises(ValueError):  # wire buffer too small
        ops.frag_pseudograd(x, x, [(0, 128)], out[:64])
    ops.frag_pseudograd(x, x, [(0, 64), (128, 192)], out)


# ------------------------------------------------------------------ 7. / 8. through the CLI
BASE = ["--llama-config-file", "configs/llama_tiny.json", "--batch-size", "8", "--per-device-batch-size", "4",
        "--seq-length", "64", "--warmup-steps", "2", "--wandb", "off", "--device", "cpu", "--debug-checks",
        "--data", "synthetic", "--total-steps", "16", "--inner-steps", "8"]
STREAM = ["--streaming-fragments", "2", "--streaming-overlap-steps", "1", "--streaming-alpha", "0.5"]


def _torchrun(nproc, args, timeout=600):
    env = child_env(OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m", "nanodiloco_amd"] + args
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _ok(r):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _tensors(path):
    from safetensors.torch import load_file
    return load_file(str(path))


@pytest.mark.slow
def test_cli_streaming_run_and_resume(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    la = tmp_path / "a.jsonl"
    r = _ok(_torchrun(2, BASE + STREAM + ["--checkpoint-dir", str(a), "--log-file", str(la)]))
    assert "Training completed!" in r.stdout
    rows = [json.loads(l) for l in open(la)]
    # the run's outer_steps: total_steps / H (the last round completes when the flush applies the fragment sent
    # after step 16; the flush's own syncs are not counted)
    ts = json.load(open(a / "trainer_state.json"))
    assert ts["outer_step_count"] == 2 and ts["outer_opt_step"] == 2
    assert rows[-1]["outer_step"] == 1 and rows[8]["outer_step"] == 1 and rows[7]["outer_step"] == 0
    frag_rows = {x["step"]: x["fragment"] for x in rows if "fragment" in x}
    assert frag_rows == {4: 0, 5: 0, 8: 1, 9: 1, 12: 0, 13: 0, 16: 1}
    assert all("bytes_outer" in x and "comm_ms" in x for x in rows if "fragment" in x)
    # after the flush: master == theta_sync, replicas identical, checkpoint export-ready
    sync = _tensors(a / "diloco_state.safetensors")["theta_sync"]
    for rk in (0, 1):
        assert torch.equal(_tensors(a / f"rank{rk}.safetensors")["master"], sync)
    assert "nanodiloco_streaming_local_weights" not in json.load(open(a / "config.json"))
    st = json.load(open(a / "trainer_state.json"))["streaming"]
    assert (st["fragments"], st["pattern"], st["overlap"], st["alpha"]) == (2, "strided", 1, 0.5)
    assert st["local_weights"] is False and st["pending_fragment"] is None

    # ---- 8. stop at step 8 (fragment 1 sent after step 8 is inside its window), resume, finish
    _ok(_torchrun(2, BASE + STREAM + ["--stop-at-step", "8", "--checkpoint-dir", str(b), "--checkpoint-every", "1"]))
    st = json.load(open(b / "trainer_state.json"))
    assert st["step"] == 8 and st["streaming"]["pending_fragment"] == 1 and st["streaming"]["pending_apply_step"] == 9
    assert json.load(open(b / "config.json"))["nanodiloco_streaming_local_weights"] is True
    for rk in (0, 1):
        per = _tensors(b / f"rank{rk}.safetensors")
        assert "master" in per and "stream.delta" in per
        sj = json.load(open(b / f"rank{rk}.json"))
        assert sj["stream_pending_fragment"] == 1 and sj["stream_apply_step"] == 9
    m0, m1 = (_tensors(b / f"rank{rk}.safetensors")["master"] for rk in (0, 1))
    assert not torch.equal(m0, m1)                                       # local weights differ per worker
    # refused: other options, no streaming flags, elastic
    other = [x if x != "2" else "1" for x in STREAM[:2]] + ["--streaming-overlap-steps", "1", "--streaming-alpha", "0.5"]
    for args, word in ((other, "fragments"), ([], "streaming"), (STREAM + ["--elastic-resume"], "elastic")):
        r = _torchrun(2, BASE + args + ["--resume", str(b)])
        assert r.returncode != 0 and word in (r.stdout + r.stderr), (args, (r.stdout + r.stderr)[-2000:])
    _ok(_torchrun(2, BASE + STREAM + ["--resume", str(b), "--checkpoint-dir", str(b)]))
    for rk in (0, 1):
        assert torch.equal(_tensors(b / f"rank{rk}.safetensors")["master"],
                           _tensors(a / f"rank{rk}.safetensors")["master"])
    for f in ("model.safetensors", "diloco_state.safetensors"):
        ta, tb = _tensors(a / f), _tensors(b / f)
        assert all(torch.equal(ta[k], tb[k]) for k in ta), f


@pytest.mark.slow
def test_cli_streaming_flags_on_plain_checkpoint_refused(tmp_path):
    ck = tmp_path / "ck"
    _ok(_torchrun(1, BASE + ["--stop-at-step", "8", "--checkpoint-dir", str(ck), "--checkpoint-every", "1"]))
    r = _torchrun(1, BASE + STREAM + ["--resume", str(ck)])
    assert r.returncode != 0 and "without streaming" in (r.stdout + r.stderr)
    _ok(_torchrun(1, BASE + ["--resume", str(ck)]))  # and loads exactly as before without the flags
