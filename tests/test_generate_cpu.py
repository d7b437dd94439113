"""Text generation on the CPU: fp32, a tiny 2-layer GQA model, the PyTorch path of every op.

Tolerance of the logit comparisons (``logit_tol``): the cached step and the recompute path evaluate the same
function in fp32 with sums taken in a different order.  The size of that effect is MEASURED on two evaluations
neither of which is the cached path -- the full forward on the whole sequence read at position t, and the full
forward on the prefix that ends at t, equal by causality -- as the largest logit difference over all t, with the
fp32 floor 2^-24 max|logit| under it (the two can agree bit for bit); 8 times that is allowed.
"""
import json
import subprocess
import sys

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.models.llama import filter_logits

from ._mp import ROOT, child_env

CFG = dict(hidden_size=64, intermediate_size=96, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
           vocab_size=101, rms_norm_eps=1e-5, max_position_embeddings=48)
N_NEW = 12


@pytest.fixture(scope="module")
def model():
    return LlamaForCausalLM(LlamaConfig.from_dict(CFG)).init_weights(5)


@pytest.fixture(scope="module")
def prompt():
    g = torch.Generator().manual_seed(3)
    return torch.randint(3, CFG["vocab_size"], (2, 7), generator=g)


@pytest.fixture(scope="module")
def runs(model, prompt):
    """(cached tokens, cached logits, recompute tokens, recompute logits), computed once."""
    a, la = model.generate(prompt, max_new_tokens=N_NEW, eos_token_id=None, return_logits=True)
    b, lb = model.generate(prompt, max_new_tokens=N_NEW, eos_token_id=None, use_cache=False, return_logits=True)
    return a, la, b, lb


@pytest.fixture(scope="module")
def logit_tol(model, runs):
    seq = runs[2]
    T0 = seq.shape[1] - N_NEW
    with torch.no_grad():
        whole = model(seq[:, :-1]).logits
        spread = 0.0
        for t in range(T0 - 1, seq.shape[1] - 1):
            spread = max(spread, float((model(seq[:, :t + 1]).logits[:, -1] - whole[:, t]).abs().max()))
    tol = 8.0 * max(spread, 2.0 ** -24 * float(whole.abs().max()))
    assert tol < 1e-4, tol  # fp32: a few 1e-6 for logits of order 1
    return tol


# ------------------------------------------------------------------------------------------ cached vs recompute
def test_cached_equals_recompute(runs, logit_tol, prompt):
    a, la, b, lb = runs
    assert a.shape == (2, 7 + N_NEW) and torch.equal(a[:, :7], prompt)
    assert la.shape == (2, N_NEW, CFG["vocab_size"]) and la.dtype == torch.float32
    worst = float((la - lb).abs().max())
    print(f"cached vs recompute: max logit difference {worst:.3e}, allowed {logit_tol:.3e}")
    assert worst <= logit_tol
    assert torch.equal(a, b)


def test_prefill_and_decode_step_by_hand(model, runs, logit_tol):
    """The three calls ``generate`` is made of; ``pos`` / ``kstart`` as documented."""
    seq, _, _, lb = runs
    T0 = seq.shape[1] - N_NEW
    cache = model.new_cache(2, T0 + 2)
    lg = model.prefill(seq[:, :T0], None, cache)
    assert cache.pos.tolist() == [T0, T0] and cache.kstart.tolist() == [0, 0] and cache.max_pos == T0
    assert float((lg - lb[:, 0]).abs().max()) <= logit_tol
    for j in range(2):
        lg = model.decode_step(seq[:, T0 + j], cache)
        assert float((lg - lb[:, j + 1]).abs().max()) <= logit_tol
    assert cache.pos.tolist() == [T0 + 2] * 2
    with pytest.raises(ValueError, match="full"):
        model.decode_step(seq[:, T0 + 2], cache)


# ------------------------------------------------------------------------------------------ HF
def test_greedy_matches_hf(model, prompt, runs, logit_tol):
    transformers = pytest.importorskip("transformers")
    hf = transformers.LlamaForCausalLM(transformers.LlamaConfig(**CFG, attn_implementation="eager")).float().eval()
    hf.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}, strict=False)
    with torch.no_grad():
        out = hf.generate(prompt, max_new_tokens=N_NEW, do_sample=False, eos_token_id=None, pad_token_id=0,
                          output_logits=True, return_dict_in_generate=True)
    # precondition on HF's own logits: no step is a near-tie, so equal functions give equal tokens
    top2 = torch.stack(out.logits, dim=1).float().topk(2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    assert gap > logit_tol, f"top-2 gap {gap:.3e} within the tolerance {logit_tol:.3e}: choose another seed"
    assert torch.equal(out.sequences, runs[0])


# ------------------------------------------------------------------------------------------ batching
def test_left_padded_batch_equals_rows_alone(model):
    g = torch.Generator().manual_seed(9)
    rows = [torch.randint(3, CFG["vocab_size"], (n,), generator=g) for n in (1, 5, 9)]
    T = 9
    ids = torch.zeros(3, T, dtype=torch.long)
    mask = torch.zeros(3, T, dtype=torch.long)
    for i, r in enumerate(rows):
        ids[i, T - len(r):] = r
        mask[i, T - len(r):] = 1
    for use_cache in (True, False):
        out = model.generate(ids, mask, max_new_tokens=8, eos_token_id=None, use_cache=use_cache)
        for i, r in enumerate(rows):
            alone = model.generate(r[None], max_new_tokens=8, eos_token_id=None, use_cache=use_cache)
            assert torch.equal(out[i, T:], alone[0, len(r):]), (use_cache, i)
    with pytest.raises(ValueError, match="left-padded"):
        model.generate(ids, mask.flip(1), max_new_tokens=2)


# ------------------------------------------------------------------------------------------ control flow
def test_eos_stops_a_row_and_pads(model, prompt, runs):
    free = runs[0][:, 7:]
    eos = int(free[0, 2])  # row 0 produces it at step 2
    assert eos not in free[1].tolist(), "choose another seed: the rows must finish at different steps"
    out = model.generate(prompt, max_new_tokens=N_NEW, eos_token_id=eos, pad_token_id=0)
    new = out[:, 7:]
    assert new.shape[1] == N_NEW  # row 1 never finishes
    first = free[0].tolist().index(eos)
    assert new[0, :first + 1].tolist() == free[0, :first + 1].tolist()
    assert new[0, first + 1:].tolist() == [0] * (N_NEW - first - 1)
    assert torch.equal(new[1], free[1])
    # every row finished: the result ends with the last row's EOS (checked every 16 steps, trimmed at the end)
    one = model.generate(prompt[:1], max_new_tokens=40, eos_token_id=eos, pad_token_id=0)
    assert one.shape[1] == 7 + first + 1 and int(one[0, -1]) == eos


def test_limits(model, prompt):
    assert model.generate(prompt, max_new_tokens=1, eos_token_id=None).shape == (2, 8)
    assert model.generate(prompt, max_new_tokens=5, eos_token_id=None).shape == (2, 12)
    with pytest.raises(ValueError, match="max_new_tokens"):
        model.generate(prompt, max_new_tokens=0)
    with pytest.raises(ValueError, match="does not fit"):
        model.prefill(prompt, None, model.new_cache(2, 6))  # a 7-token prompt, 6 slots
    with pytest.raises(ValueError, match="max_position_embeddings"):
        model.new_cache(2, CFG["max_position_embeddings"] + 1)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        model.generate(prompt, max_new_tokens=CFG["max_position_embeddings"])
    with pytest.raises(ValueError, match="max_position_embeddings"):
        model.generate(prompt, max_new_tokens=CFG["max_position_embeddings"], use_cache=False)
    # exactly full is fine: the last token drawn needs no slot
    full = model.generate(prompt, max_new_tokens=CFG["max_position_embeddings"] - 7 + 1, eos_token_id=None)
    assert full.shape[1] == CFG["max_position_embeddings"] + 1


# ------------------------------------------------------------------------------------------ sampling
def _filter64(row, top_k, top_p):
    """Brute force in float64, one row: the definition in ``filter_logits``'s docstring, no sort of ties involved."""
    x = [float(v) for v in row]
    keep = [True] * len(x)
    if 0 < top_k < len(x):
        kth = sorted(x, reverse=True)[top_k - 1]
        keep = [v >= kth for v in x]
    if top_p < 1.0:
        vals = [v for v, k in zip(x, keep) if k]
        m = max(vals)
        z = sum(torch.tensor([v - m for v in vals], dtype=torch.float64).exp().tolist())
        thr = None
        for v in sorted(set(vals), reverse=True):  # a token is kept when the mass of the larger logits is < top_p
            before = sum(torch.tensor([u - m for u in vals if u > v], dtype=torch.float64).exp().tolist()) / z
            # tokens equal to v: the first of them has `before` in front of it -- kept if that is < top_p, and then
            # all its ties stay with it
            if before < top_p:
                thr = v
        keep = [k and v >= thr for v, k in zip(x, keep)]
    return keep


def test_filter_logits_against_brute_force():
    # probabilities are dyadic (logits = log2-spaced) so that fp32 and float64 masses compare equal at thresholds
    ln2 = torch.log(torch.tensor(2.0, dtype=torch.float64))
    base = (torch.tensor([-1.0, -2.0, -3.0, -4.0, -5.0, -6.0, -7.0, -7.0, -3.0, -2.0], dtype=torch.float64) * ln2).float()
    g = torch.Generator().manual_seed(0)
    rows = torch.stack([base, base[torch.randperm(10, generator=g)], torch.randn(10, generator=g),
                        torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0, -1.0, 2.0, 2.0, -3.0, 0.5])])
    for top_k in (0, 1, 2, 3, 5, 10, 50):
        for top_p in (1.0, 0.9, 0.5, 0.26, 0.05):
            got = filter_logits(rows, top_k, top_p)
            for r in range(rows.shape[0]):
                keep = _filter64(rows[r], top_k, top_p)
                assert (got[r] > float("-inf")).tolist() == keep, (top_k, top_p, r)
                assert torch.equal(got[r][torch.tensor(keep)], rows[r][torch.tensor(keep)])
    # ties at the top-k threshold are all kept
    assert int((filter_logits(rows[3:], 1, 1.0) > float("-inf")).sum()) == 2


def test_sampling(model, prompt, runs):
    greedy = runs[0][:, :7 + 6]
    for temp in (0.3, 1.0, 2.5):
        assert torch.equal(model.generate(prompt, max_new_tokens=6, temperature=temp, top_k=1, eos_token_id=None,
                                          seed=4), greedy)
    kw = dict(max_new_tokens=N_NEW, temperature=1.0, eos_token_id=None)
    a = model.generate(prompt, seed=1, **kw)
    assert torch.equal(a, model.generate(prompt, seed=1, **kw))
    assert torch.equal(a, model.generate(prompt, seed=1, use_cache=False, **kw))
    assert not torch.equal(a, model.generate(prompt, seed=2, **kw))
    assert not torch.equal(a, runs[0])
    # top-k restricts the draw: every sampled token is among the step's 3 best
    out, lg = model.generate(prompt, seed=5, top_k=3, return_logits=True, **kw)
    best = lg.topk(3, dim=-1).indices
    assert bool((best == out[:, 7:, None]).any(-1).all())


# ------------------------------------------------------------------------------------------ training isolation
def test_generate_leaves_training_state(prompt):
    m = LlamaForCausalLM(LlamaConfig.from_dict(CFG)).init_weights(5)
    m(prompt, labels=prompt).loss.backward()
    grad, version = m.store.grad.clone(), m.store.version
    master = m.store.master.clone() if hasattr(m.store, "master") else None
    assert m.training
    m.generate(prompt, max_new_tokens=4, eos_token_id=None)
    m.generate(prompt, max_new_tokens=4, eos_token_id=None, use_cache=False, temperature=1.0)
    assert m.training and m.store.version == version and torch.equal(m.store.grad, grad)
    if master is not None:
        assert torch.equal(m.store.master, master)
    m.eval()
    m.generate(prompt, max_new_tokens=2, eos_token_id=None)
    assert not m.training


# ------------------------------------------------------------------------------------------ CLI
def test_cli_round_trip(tmp_path):
    from nanodiloco_amd.trainer import TrainArgs, Trainer
    from nanodiloco_amd.utils.checkpoint import _load_st, find_checkpoint
    ck = tmp_path / "ck"
    tr = Trainer(TrainArgs(llama_config_file="configs/llama_tiny.json", batch_size=4, per_device_batch_size=4,
                           seq_length=32, warmup_steps=1, total_steps=2, inner_steps=2, wandb="off", device="cpu",
                           data="synthetic", log_every=1, checkpoint_dir=str(ck), seed=3))
    tr.train()
    pf = tmp_path / "prompts.jsonl"
    pf.write_text("[5, 6, 7, 8, 9]\n")
    r = subprocess.run([sys.executable, "-m", "nanodiloco_amd.generate", "--checkpoint", str(ck), "--prompt-ids",
                        "1,2,3", "--prompt-file", str(pf), "--max-new-tokens", "6", "--device", "cpu"], cwd=ROOT,
                       env=child_env(OMP_NUM_THREADS=str(torch.get_num_threads())), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.strip().splitlines()]
    assert len(lines) == 3
    assert lines[0]["prompt_ids"] == [1, 2, 3] and lines[1]["prompt_ids"] == [5, 6, 7, 8, 9]
    assert set(lines[2]) == {"prefill_s", "decode_s", "decode_tokens_per_s"}
    # the API on the same weights
    path = find_checkpoint(str(ck))
    cfg = LlamaConfig.from_json(f"{path}/config.json")
    m = LlamaForCausalLM(cfg, "cpu", torch.float32)
    m.load_state_dict(_load_st(f"{path}/model.safetensors"))
    eos = cfg.eos_token_id
    for rec in lines[:2]:
        p = rec["prompt_ids"]
        want = m.generate(torch.tensor([p]), max_new_tokens=6)[0].tolist()
        assert rec["token_ids"] == want and rec["new_tokens"] == len(want) - len(p) <= 6
        assert eos not in rec["token_ids"][len(p):-1]
    # without a tokenizer text is refused
    r = subprocess.run([sys.executable, "-m", "nanodiloco_amd.generate", "--checkpoint", str(ck), "--prompt", "hi"],
                       cwd=ROOT, env=child_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--tokenizer" in r.stderr
