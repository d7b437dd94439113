"""Held-out evaluation on the CPU: the loss-only lm head's torch twin against the training forward, the CLI flags,
the eval stream (fixed, apart from the training stream), the training trajectory with and without evaluation, two
gloo workers, and the stand-alone ``python -m nanodiloco_amd.evaluate`` against the run's own final number."""
import json
import os
import subprocess
import sys

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import resolve_llama_config
from nanodiloco_amd.data import build_data, build_eval_data
from nanodiloco_amd.data.memmap import write_token_shard
from nanodiloco_amd.main import parse_args
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.trainer import TrainArgs, Trainer

from ._mp import ROOT, child_env, run_ranks

TINY = "configs/llama_tiny.json"
B, T = 4, 64


def _targs(**kw):
    base = dict(llama_config_file=TINY, batch_size=8, per_device_batch_size=B, seq_length=T, warmup_steps=2,
                total_steps=6, inner_steps=3, wandb="off", device="cpu", data="synthetic", log_every=1)
    base.update(kw)
    return TrainArgs(**base)


def _log(path):
    return [json.loads(l) for l in open(path)]


# ------------------------------------------------------------------------------------------ twin vs training forward
def test_twin_matches_training_forward():
    """CPU fp32: loss_stats and model(input_ids, labels).loss are the same fp32 row losses, one summed in fp64 and
    one in fp32: they agree to n_valid * 2^-24 * |loss|.  row_hit is argmax == target wherever the top two logits
    differ."""
    torch.manual_seed(0)
    cfg = resolve_llama_config(TINY)
    model = LlamaForCausalLM(cfg, "cpu", torch.float32).init_weights(3)
    ids = torch.randint(0, cfg.vocab_size, (2, T))
    labels = ids.clone()
    labels[0, 5:9] = -100
    st = model.loss_stats(ids, labels)
    assert st.dtype == torch.float64 and st.shape == (3,)
    assert model.training
    with torch.no_grad():
        out = model(ids, labels=labels, return_logits=True)
    n_valid = int(st[1])
    targets = ops.reference.shift_labels(labels).reshape(-1)
    assert n_valid == int((targets != -100).sum()) == 2 * (T - 1) - 4
    loss = float(out.loss)
    assert abs(float(st[0]) / n_valid - loss) <= n_valid * 2.0 ** -24 * abs(loss)
    # the op itself, row by row
    y = model.hidden_states(ids).detach()
    lm = "lm_head.weight" if not cfg.tie_word_embeddings else "model.embed_tokens.weight"
    row_loss, row_hit = ops.lm_head_loss(y, model._w(lm), targets)
    assert row_loss.dtype == torch.float32 and row_hit.dtype == torch.bool
    logits = out.logits.reshape(-1, cfg.vocab_size)
    top2 = logits.topk(2, dim=-1).values
    clear = top2[:, 0] != top2[:, 1]
    ok = targets != -100
    want = ok & (logits.argmax(-1) == targets)
    assert bool(clear.any()) and torch.equal(row_hit[clear], want[clear])
    assert not bool(row_hit[~ok].any()) and not bool(row_loss[~ok].any())
    assert int(st[2]) == int(row_hit.sum())


def test_lm_head_loss_chunks_agree():
    torch.manual_seed(1)
    y, w = torch.randn(600, 32), torch.randn(100, 32)
    tgt = torch.randint(0, 100, (600,))
    tgt[256:512] = -100
    a = ops.lm_head_loss(y, w, tgt)
    b = ops.lm_head_loss(y, w, tgt, chunk_rows=256)
    assert torch.allclose(a[0], b[0], rtol=0, atol=1e-5) and torch.equal(a[1], b[1])
    assert not bool(b[0][256:512].any()) and not bool(b[1][256:512].any())


# ------------------------------------------------------------------------------------------ CLI
def test_cli_flags_and_defaults():
    a = parse_args([])
    assert a.eval_every == 0 and a.eval_batches == 8 and a.eval_dataset_path is None
    a = parse_args(["--eval-every", "50", "--eval-batches", "3", "--eval-dataset-path", "/x/heldout"])
    assert a.eval_every == 50 and a.eval_batches == 3 and a.eval_dataset_path == "/x/heldout"


def test_eval_off_builds_no_stream():
    tr = Trainer(_targs())
    assert tr.eval_data is None
    assert "final_eval_loss" not in tr.train()


def test_memmap_without_eval_path_raises(tmp_path):
    write_token_shard(str(tmp_path / "train.bin"), torch.randint(0, 1000, (B * T * 8,)).numpy(), 1024)
    with pytest.raises(ValueError, match="eval-dataset-path"):
        Trainer(_targs(data="memmap", dataset_path=str(tmp_path), eval_every=2))
    Trainer(_targs(data="memmap", dataset_path=str(tmp_path)))  # without evaluation the same run is fine


def test_hf_with_eval_raises():
    with pytest.raises(NotImplementedError, match="not supported yet"):
        build_eval_data("hf", vocab_size=1024, seq_len=T, batch_size=B, seed=1, rank=0, world_size=1, device="cpu")


# ------------------------------------------------------------------------------------------ the eval stream
def _take(stream, k):
    stream.reset()
    return [next(stream)["input_ids"].clone() for _ in range(k)]


def _kw(**kw):
    base = dict(vocab_size=1024, seq_len=T, batch_size=B, seed=7, rank=0, world_size=1, device="cpu")
    base.update(kw)
    return base


def test_synthetic_eval_stream_fixed_and_apart():
    ev = build_eval_data("synthetic", **_kw())
    a, b = _take(ev, 3), _take(ev, 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], a[1])
    train = build_data("synthetic", **_kw())
    assert not torch.equal(next(train)["input_ids"], a[0])  # stream 2, not the training stream 1
    other = build_eval_data("synthetic", **_kw(rank=1, world_size=2))
    assert not torch.equal(_take(other, 1)[0], a[0])


def test_memmap_eval_stream_fixed_and_disjoint(tmp_path):
    nwin = 64
    toks = torch.arange(nwin * T) % 1000  # window w starts with token (w * T) % 1000: windows are tell-apart
    write_token_shard(str(tmp_path / "heldout.bin"), toks.numpy(), 1024)
    ev = build_eval_data("memmap", **_kw(eval_dataset_path=str(tmp_path)))
    a, b = _take(ev, 3), _take(ev, 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    r0 = build_eval_data("memmap", **_kw(world_size=2, eval_dataset_path=str(tmp_path)))
    r1 = build_eval_data("memmap", **_kw(rank=1, world_size=2, eval_dataset_path=str(tmp_path / "*.bin")))
    k = 3
    w0 = {r0.source.window_of(i) for i in range(k * B)}
    w1 = {r1.source.window_of(i) for i in range(k * B)}
    assert len(w0) == len(w1) == k * B and not (w0 & w1)
    rows0 = {tuple(r.tolist()) for t in _take(r0, k) for r in t}
    rows1 = {tuple(r.tolist()) for t in _take(r1, k) for r in t}
    assert not (rows0 & rows1)


def test_training_stream_untouched_by_evaluation():
    tr = Trainer(_targs(eval_every=2, eval_batches=2))
    next(tr.data)
    before = tr.data.state_dict()
    tr.evaluate()
    after = tr.data.state_dict()
    assert before["samples_drawn"] == after["samples_drawn"]
    assert torch.equal(before["gen_state"], after["gen_state"])


# ------------------------------------------------------------------------------------------ trajectory
def test_evaluation_does_not_move_training(tmp_path):
    ref = Trainer(_targs())
    ref.train()
    log = tmp_path / "m.jsonl"
    tr = Trainer(_targs(eval_every=2, eval_batches=2, log_file=str(log)))
    out = tr.train()
    assert torch.equal(ref.model.store.master, tr.model.store.master)
    recs = [r for r in _log(log) if "eval_loss" in r]
    for r in recs:
        assert {"eval_loss", "eval_perplexity", "eval_accuracy", "eval_tokens", "eval_s", "step"} <= set(r)
        assert "loss" not in r  # a record of its own
        assert r["eval_tokens"] == 1 * 2 * B * (T - 1)
        assert 0.0 <= r["eval_accuracy"] <= 1.0 and r["eval_loss"] > 0
    # 2, 4 in the loop; 6 once, after finalize
    assert [r["step"] for r in recs] == [2, 4, 6]
    assert out["final_eval_loss"] == recs[-1]["eval_loss"]


def test_final_evaluation_when_not_a_multiple():
    tr = Trainer(_targs(eval_every=4, eval_batches=1))
    seen = []
    orig = tr.evaluate
    tr.evaluate = lambda step=None: (seen.append(step), orig(step))[1]
    out = tr.train()
    assert seen == [4, 6] and "final_eval_loss" in out


def test_stop_at_step_has_no_final_evaluation():
    tr = Trainer(_targs(eval_every=2, eval_batches=1, stop_at_step=4))
    seen = []
    orig = tr.evaluate
    tr.evaluate = lambda step=None: (seen.append(step), orig(step))[1]
    out = tr.train()
    assert seen == [2, 4] and "final_eval_loss" not in out


# ------------------------------------------------------------------------------------------ two workers
def _rank_eval(rank, world):
    from nanodiloco_amd.trainer import TrainArgs, Trainer
    torch.set_num_threads(2)
    tr = Trainer(TrainArgs(llama_config_file=TINY, batch_size=8, per_device_batch_size=B, seq_length=T, warmup_steps=2,
                           total_steps=6, inner_steps=3, wandb="off", device="cpu", data="synthetic", backend="gloo",
                           eval_every=3, eval_batches=2))
    rec = tr.evaluate()
    # this rank's own share, without the collective
    tr.eval_data.reset()
    acc = torch.zeros(3, dtype=torch.float64)
    for _ in range(2):
        b = next(tr.eval_data)
        acc += tr.model.loss_stats(b["input_ids"], b["labels"])
    return rec["eval_loss"], rec["eval_tokens"], acc.tolist()


@pytest.mark.slow
def test_two_workers_token_weighted():
    res = run_ranks(_rank_eval, 2)
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    s = [r[2] for r in res]
    assert s[0] != s[1]  # different held-out data per rank
    want = (s[0][0] + s[1][0]) / (s[0][1] + s[1][1])
    assert res[0][1] == int(s[0][1] + s[1][1]) == 2 * 2 * B * (T - 1)
    assert abs(res[0][0] - want) <= 4 * 2.0 ** -53 * abs(want)


# ------------------------------------------------------------------------------------------ stand-alone
@pytest.mark.slow
def test_standalone_matches_final_eval(tmp_path):
    ck = tmp_path / "ck"
    tr = Trainer(_targs(total_steps=4, inner_steps=2, eval_every=4, eval_batches=2, checkpoint_dir=str(ck), seed=11))
    out = tr.train()
    r = subprocess.run([sys.executable, "-m", "nanodiloco_amd.evaluate", "--checkpoint", str(ck), "--data", "synthetic",
                        "--eval-batches", "2", "--per-device-batch-size", str(B), "--seq-length", str(T), "--seed",
                        "11", "--device", "cpu"], cwd=ROOT, env=child_env(OMP_NUM_THREADS=str(torch.get_num_threads())),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["eval_loss"] == out["final_eval_loss"]
    assert rec["eval_tokens"] == 2 * B * (T - 1)
    assert not os.path.exists(str(ck) + ".tmp")
