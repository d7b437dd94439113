#!/usr/bin/env python
"""Multi-token KV-cache attention and chunked prefill, timed on the GPU.

  kernel : ``nd_attn_extend`` (ops.decode.attn_extend_launch), one call that appends L = 64 tokens per sequence, against
           64 successive ``nd_attn_decode`` steps over the same tokens (the only way to do it before), at the
           Llama-150M head shape (nh 16, nkv 16, hd 64), B = 4, the block ending at slot 2048 of an S_max = 2048
           cache.  Timed interleaved in one process, round by round, device events around ``--inner`` back-to-back
           repetitions after a warm-up; per-repetition median and minimum over the rounds.  Both must agree (max
           difference printed; different kernels, not bitwise).
  e2e    : ``model.generate`` of Llama-150M (random weights), one new token after a 2048-token prompt, B = 1:
           ``prefill_chunk`` 0 (the training forward over the whole prompt) vs 64 (``model.extend`` in pieces), a host
           clock around the call with a device synchronise, rounds interleaved.

    python scripts/extend_bench.py [--rounds 20] [--inner 10] [--e2e-rounds 5] [--skip-e2e] [--out FILE.json]

Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.ops import decode  # noqa: E402
from nanodiloco_amd.ops.attention import rope_cache  # noqa: E402

NH, NKV, HD, S_MAX, B, L = 16, 16, 64, 2048, 4, 64


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner, out


def bench_kernel(rounds, inner, dev):
    g = torch.Generator(device=dev).manual_seed(5)
    kc = torch.randn(B, NKV, S_MAX, HD, device=dev, generator=g).bfloat16()
    vc = torch.randn(B, NKV, S_MAX, HD, device=dev, generator=g).bfloat16()
    qkv = torch.randn(B * L, (NH + 2 * NKV) * HD, device=dev, generator=g).bfloat16()
    cos, sin = rope_cache(S_MAX, HD, 10000.0, None, dev)
    p0 = S_MAX - L
    pos = torch.full((B,), p0, dtype=torch.int32, device=dev)
    steps = [torch.full((B,), p0 + i, dtype=torch.int32, device=dev) for i in range(L)]
    rows = [qkv.view(B, L, -1)[:, i].contiguous() for i in range(L)]
    ks = torch.zeros(B, dtype=torch.int32, device=dev)
    xo, xml = decode.extend_workspace(B, NH, HD, S_MAX, dev)
    do, dml = decode.decode_workspace(B, NH, HD, S_MAX, dev)
    scratch = torch.empty_like(qkv)

    def extend():
        scratch.copy_(qkv)  # the launch rotates its input in place
        return decode.attn_extend_launch(scratch, cos, sin, pos, ks, kc, vc, xo, xml, L, NH, NKV, HD).view(B, L, -1)

    def copy_only():
        scratch.copy_(qkv)
        return scratch

    def loop():
        return torch.stack([decode.attn_decode_launch(rows[i], cos, sin, steps[i], ks, kc, vc, do, dml, NH, NKV, HD)
                            for i in range(L)], 1)

    fns = {"extend": extend, "decode_x64": loop, "input_copy": copy_only}
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms, vals = {k: [] for k in fns}, {}
    for _ in range(rounds):
        for k, f in fns.items():
            t, o = timed(f, inner)
            ms[k].append(t)
            vals[k] = o.float().clone()
    r = {"B": B, "L": L, "cache": S_MAX, "rounds": rounds, "inner": inner,
         "max_diff": float((vals["extend"] - vals["decode_x64"]).abs().max())}
    for k, v in ms.items():
        r[k + "_us_median"], r[k + "_us_min"] = 1e3 * statistics.median(v), 1e3 * min(v)
    return r


def bench_e2e(rounds, dev):
    from nanodiloco_amd.config import resolve_llama_config
    from nanodiloco_amd.models import LlamaForCausalLM
    cfg = resolve_llama_config("llama_150m.json")
    m = LlamaForCausalLM(cfg, dev, torch.bfloat16).init_weights(1)
    ids = torch.randint(3, cfg.vocab_size, (1, 2048), generator=torch.Generator().manual_seed(2)).to(dev)
    sec = {0: [], 64: []}
    for rnd in range(rounds + 1):  # round 0 is the warm-up
        for chunk in sec:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(ids, max_new_tokens=1, eos_token_id=None, hip_graph=False, prefill_chunk=chunk)
            torch.cuda.synchronize()
            if rnd:
                sec[chunk].append(time.perf_counter() - t0)
    return {f"prefill_chunk_{c}_ms_median": 1e3 * statistics.median(v) for c, v in sec.items()} | \
           {f"prefill_chunk_{c}_ms_min": 1e3 * min(v) for c, v in sec.items()} | {"prompt": 2048, "B": 1, "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--e2e-rounds", type=int, default=5)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("extend_bench needs a GPU")
    ops.set_backend("hip")
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"kernel": bench_kernel(a.rounds, a.inner, dev)}
    print(json.dumps(res["kernel"]), flush=True)
    if not a.skip_e2e:
        res["e2e"] = bench_e2e(a.e2e_rounds, dev)
        print(json.dumps(res["e2e"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
