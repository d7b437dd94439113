"""The on-disk contract of a checkpoint, per outer transport: which tensors every ``rank*.safetensors`` holds and
which keys ``rank*.json``, ``trainer_state.json`` and ``config.json`` have, each saved in the state that transport
alone can be in (an overlapped outer step pending, error-feedback residuals, a fragment in flight).  The lists are
what the commit before the transports were split (parallel/transports.py) wrote for the same runs: a checkpoint of
either side of that change must load on the other."""
import json
import os

import pytest
import torch
from safetensors import safe_open

from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
from nanodiloco_amd.parallel.diloco import Diloco
from nanodiloco_amd.parallel.dist import DistEnv
from nanodiloco_amd.utils.checkpoint import save_checkpoint

TINY4 = dict(hidden_size=32, intermediate_size=64, num_attention_heads=2, num_hidden_layers=4, vocab_size=50,
             rms_norm_eps=1e-5)
H = 8
HF_CONFIG = ["architectures", "attention_bias", "attention_dropout", "bos_token_id", "eos_token_id", "head_dim",
             "hidden_act", "hidden_size", "initializer_range", "intermediate_size", "max_position_embeddings",
             "mlp_bias", "model_type", "num_attention_heads", "num_hidden_layers", "num_key_value_heads",
             "pad_token_id", "pretraining_tp", "rms_norm_eps", "rope_scaling", "rope_theta", "tie_word_embeddings",
             "torch_dtype", "use_cache", "vocab_size"]
ADAMW = ["adamw.exp_avg", "adamw.exp_avg_sq"]
TRAINER = ["flat_numel", "inner_dp", "local_step", "outer_opt_step", "outer_step_count", "pending_outer",
           "scheduler", "step", "world_size"]
# options, the inner step to save after, then the expected names
CASES = {
    "dense_overlap_pending": (dict(overlap=True), 8, {
        "rank0.safetensors": ADAMW + ["master", "outer.delta", "outer.drift_base"],
        "rank0.json": ["adamw_step"],
        "trainer_state.json": TRAINER,
        "config.json": HF_CONFIG + ["nanodiloco_pending_outer_step"]}),
    "int8_error_feedback": (dict(comm_dtype="int8", error_feedback=True, bucket_mb=4096 / (1 << 20)), 8, {
        "rank0.safetensors": ADAMW + ["qef.reduce", "qef.send"],
        "rank0.json": ["adamw_step"],
        "trainer_state.json": TRAINER + ["comm_error_feedback"],
        "trainer_state.json:comm_error_feedback": ["bits", "num_workers", "plan"],
        "config.json": HF_CONFIG}),
    "streaming_fragment_in_flight": (dict(fragments=2, stream_overlap=2, stream_alpha=0.5), 5, {
        "rank0.safetensors": ADAMW + ["master", "stream.delta"],
        "rank0.json": ["adamw_step", "stream_apply_step", "stream_pending_fragment"],
        "trainer_state.json": TRAINER + ["streaming"],
        "trainer_state.json:streaming": ["alpha", "frag_steps", "fragment_sync_count", "fragments", "local_weights",
                                         "overlap", "pattern", "pending_apply_step", "pending_fragment"],
        "config.json": HF_CONFIG + ["nanodiloco_streaming_local_weights"]}),
}


def _names(ckpt):
    """{file: sorted tensor names or JSON keys}, plus the keys of the per-transport records of trainer_state.json"""
    out = {}
    for f in os.listdir(ckpt):
        path = os.path.join(ckpt, f)
        if f.startswith("rank") and f.endswith(".safetensors"):
            with safe_open(path, "pt") as sf:
                out[f] = sorted(sf.keys())
        elif f in ("trainer_state.json", "config.json") or (f.startswith("rank") and f.endswith(".json")):
            with open(path) as fh:
                rec = json.load(fh)
            out[f] = sorted(rec)
            out.update({f"{f}:{k}": sorted(v) for k, v in rec.items() if isinstance(v, dict) and k != "scheduler"})
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_names_on_disk(case, tmp_path):
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    kw, at, want = CASES[case]
    m = LlamaForCausalLM(LlamaConfig.from_dict(TINY4)).init_weights(3)
    d = Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store, lr=0.7, momentum=0.9), 2, 4 * H, H,
               env=DistEnv(), **kw)
    for t in range(1, at + 1):
        ids = torch.randint(0, 50, (2, 16), generator=torch.Generator().manual_seed(t))
        m(ids, labels=ids).loss.backward()
        d.inner_step()
        if kw.get("fragments"):
            d.stream_step(t)
        elif t % H == 0:
            d.outer_step()
    save_checkpoint(str(tmp_path / "ck"), m, d, DistEnv(), step=at)
    got = _names(str(tmp_path / "ck"))
    assert got == {f: sorted(names) for f, names in want.items()}
    assert sorted(os.listdir(tmp_path / "ck")) == ["COMPLETE.json", "config.json", "diloco_state.safetensors",
                                                   "model.safetensors", "rank0.json", "rank0.safetensors",
                                                   "trainer_state.json"]
