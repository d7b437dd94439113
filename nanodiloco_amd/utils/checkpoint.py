"""Checkpoint / resume (the reference has none -- SURVEY.md §5.4 -- so the format is defined here).

Directory layout (written only at outer-step boundaries, when all replicas are identical):

  <dir>/config.json              HF LlamaConfig JSON (+ "architectures": ["LlamaForCausalLM"]); a soft-capped model
                                 also carries "final_logit_softcapping": C, which ``--resume``, ``evaluate`` and
                                 ``generate`` apply and stock ``transformers`` Llama ignores (docs/MIGRATING.md)
  <dir>/model.safetensors        fp32 master weights, HF key names -> ``LlamaForCausalLM.from_pretrained(dir)``
  <dir>/diloco_state.safetensors outer state shared by all workers: theta_sync, outer momentum
  <dir>/rank{r}.safetensors      per-rank inner AdamW m/v + data-generator state (``--inner-optimizer muon``: the
                                 same two tensors, the Muon momentum in ``adamw.exp_avg`` over the Muon spans;
                                 ``trainer_state.json`` then records ``"inner_optimizer": "muon"`` and resume refuses
                                 a mismatch; a checkpoint without the key is ``adamw``)
  <dir>/trainer_state.json       step counters, schedule, hyper-params, topology (world size, inner_dp,
                                 flat size -- validated on resume), per-rank scalar state

With ``--overlap-outer`` a checkpoint taken at an outer boundary holds that step still PENDING (its
all-reduce finished, its one-step-late application not yet done): the reduced pseudo-gradient and each
rank's drift base and local weights go into the rank files, and the resumed run applies the step after its first inner
step -- the same trajectory as the uninterrupted run (tests/test_e2e_cpu.py).  Such an INTERMEDIATE checkpoint is
not export-ready: its model.safetensors holds rank 0's local weights (drifted by that worker's inner progress,
without the pending outer update), and config.json says so (``"nanodiloco_pending_outer_step": true``).  For
evaluation / export use a checkpoint without that flag -- the final one (``Diloco.finalize`` applies the
pending step first) or any checkpoint of a run without ``--overlap-outer``.

With ``--streaming-fragments`` (Streaming DiLoCo) the local weights of the workers differ between the first fragment
sync and ``Diloco.flush_fragments``: every rank file carries its ``master``; when a fragment is inside its overlap
window, also ``stream.delta`` (the reduced packed pseudo-gradient) and, in ``rank{r}.json``, the pending fragment
index with its apply step, so the resumed run applies it at the same step.  ``trainer_state.json`` records
``streaming: {fragments, pattern, overlap, alpha, frag_steps, ...}`` -- resume refuses a mismatch of any of the four
options, a streaming checkpoint without the flags (and the converse) and ``--elastic-resume`` -- and ``config.json``
says ``"nanodiloco_streaming_local_weights": true`` (not export-ready, like the pending-step flag).  The final
checkpoint is written after the flush and carries neither.

What depends on the outer transport is given and taken by ``Diloco.transport`` (parallel/transports.py:
``rank_state`` / ``shared_state`` / ``load_state``), under the names this text gives.

With ``--comm-error-feedback`` (quantised transport with residuals) every rank file carries
``qef.send`` and ``qef.reduce``, and ``trainer_state.json`` records ``comm_error_feedback: {bits, num_workers, plan}``
(the bucket plan ``[[x, y, c], ...]`` that ``qef.reduce`` is laid out by).  The residuals are an optimisation state
that may be dropped (``QuantisedTransport.load_error_feedback_state`` has the rules and the cost): a stateless
checkpoint resumes with the flag on from zero residuals, a checkpoint with residuals resumes without the flag and ignores
them, ``qef.send`` survives int8 <-> int4 and ``--elastic-resume`` (surviving ranks; new workers start at zero),
``qef.reduce`` only an unchanged plan and worker count.

With ``--comm-topk K`` (top-k sparse transport) every rank file carries ``topk.residual`` (fp32, one element per
element of the span the rank owns) and ``trainer_state.json`` records ``comm_topk: {k, chunk, value_dtype}``.  The
residual is an amount still owed, whatever it was selected with: it is restored whenever its length matches (another K,
another value dtype, another number of workers), else the rank starts from zero with a logged line; a rank without one
starts at zero, and a run without ``--comm-topk`` ignores it with a logged line (``TopKTransport.load_state``).

With ``--comm-rank R`` (low-rank transport) every rank file carries ``lowrank.residual`` (fp32, one element per element
of the flat vector, zero on the dense spans), ``diloco_state.safetensors`` carries ``lowrank.q`` (the Q factors, the same
on every worker: ``transport.shared_tensors()``) and ``trainer_state.json`` records ``comm_lowrank: {rank, seed}``.  The
residual is restored whenever its length matches, also under another R (logged); Q only when R and the seed are the
checkpoint's, else it is re-seeded (logged) -- Q0 is regenerated from the seed and never saved; a run without
``--comm-rank`` ignores both with a logged line (``LowRankTransport.load_state``).

Crash consistency (round 5): every rank writes into ``<dir>.tmp``; after a barrier rank 0 adds
``COMPLETE.json`` and swaps the staging directory in (``<dir>`` -> ``<dir>.old``, ``<dir>.tmp`` -> ``<dir>``,
then ``<dir>.old`` is removed), so a crash at any point of a save leaves the previous complete checkpoint
readable (``find_checkpoint`` falls back to ``<dir>.old`` when the swap itself was interrupted).  ``--resume
auto`` resumes from the newest complete checkpoint in ``--checkpoint-dir`` if there is one and starts fresh
otherwise -- the restart form for ``torchrun --max-restarts N`` (tests/test_e2e_cpu.py
injects a crash with ``ND_FAULT_INJECT``).

Only safetensors + JSON: nothing executable is ever deserialised.
"""
from __future__ import annotations

import json
import os
import shutil
from typing import Any, Dict, Optional

import torch

from ..parallel.dist import DistEnv, barrier


COMPLETE = "COMPLETE.json"


def _stage_dir(ckpt_dir: str) -> str:
    return os.path.normpath(ckpt_dir) + ".tmp"


def find_checkpoint(ckpt_dir: Optional[str]) -> Optional[str]:
    """The newest COMPLETE checkpoint for ``ckpt_dir``: itself; else the staging ``<dir>.tmp`` when a save was
    interrupted after its COMPLETE marker but before its swap finished (newer than ``<dir>.old``); else
    ``<dir>.old``; else a pre-round-5 checkpoint without the marker; else None."""
    if not ckpt_dir:
        return None
    d = os.path.normpath(ckpt_dir)
    for cand in (d, _stage_dir(d), d + ".old"):
        if os.path.isfile(os.path.join(cand, COMPLETE)):
            return cand
    if os.path.isfile(os.path.join(d, "trainer_state.json")) and not os.path.exists(_stage_dir(d)):
        return d  # written before the staging scheme existed
    return None


def _swap_in(stage: str, final: str) -> None:
    """Make the complete ``stage`` the checkpoint.  At every instant some complete copy is where
    :func:`find_checkpoint` looks: ``final`` (or ``stage``, or ``final.old``) -- a leftover ``.old`` is deleted
    only while a complete ``final`` exists, and with no ``final`` the stage moves in before anything is deleted."""
    old = final + ".old"
    if os.path.isdir(final):
        if os.path.isdir(old):
            shutil.rmtree(old)
        os.replace(final, old)
    os.replace(stage, final)
    shutil.rmtree(old, ignore_errors=True)


def _save_st(path: str, tensors: Dict[str, torch.Tensor]):
    from safetensors.torch import save_file

    save_file({k: v.detach().contiguous().cpu() for k, v in tensors.items()}, path + ".tmp")
    os.replace(path + ".tmp", path)


def _load_st(path: str) -> Dict[str, torch.Tensor]:
    from safetensors.torch import load_file

    return load_file(path)


def inner_optimizer_kind(opt) -> str:
    """``"muon"`` for ``optim.FlatMuon`` (its ``exp_avg`` holds Muon momentum over the Muon spans), else ``"adamw"``."""
    from ..optim import FlatMuon
    return "muon" if isinstance(opt, FlatMuon) else "adamw"


def save_checkpoint(ckpt_dir: str, model, diloco, env: DistEnv, step: int, data_state: Optional[Dict[str, Any]] = None,
                    extra: Optional[Dict[str, Any]] = None):
    # a collective still in flight (overlapped step, fragment) is waited for and saved as pending, not applied
    t_per, t_scal = diloco.transport.rank_state()
    shared, export_flags = diloco.transport.shared_state()
    if env.inner_dp > 1:
        # two-level mode: each GPU of a worker updates only its shard of the outer momentum
        # (parallel/diloco.py, sharded outer step); gather the worker's full buffer before rank 0
        # writes it, so a resumed run restores every shard (not just shard 0)
        diloco.inner_comm.all_gather_flat(diloco.outer_optimizer.momentum_buffer, diloco.shards, env.inner_rank)
    final = os.path.normpath(ckpt_dir)
    ckpt_dir = _stage_dir(final)  # every file below goes to the staging directory
    r = env.rank
    if r == 0:
        shutil.rmtree(ckpt_dir, ignore_errors=True)  # leftovers of a save that crashed
        os.makedirs(ckpt_dir)
    barrier(env)
    store = model.store
    # per-rank state (every rank)
    per = {"adamw.exp_avg": diloco.inner_optimizer.exp_avg, "adamw.exp_avg_sq": diloco.inner_optimizer.exp_avg_sq,
           **t_per}
    scal: Dict[str, Any] = {"adamw_step": diloco.inner_optimizer.step_count, **t_scal}
    if data_state:
        for k, v in data_state.items():
            if isinstance(v, torch.Tensor):
                per[f"data.{k}"] = v
            else:
                scal[f"data.{k}"] = v
    _save_st(os.path.join(ckpt_dir, f"rank{r}.safetensors"), per)
    with open(os.path.join(ckpt_dir, f"rank{r}.json"), "w") as f:
        json.dump(scal, f)
    if r == 0:
        cfg_json = model.config.to_hf_json()
        cfg_json.update(export_flags)  # see the module doc: rank 0's local weights, not the synced model
        with open(os.path.join(ckpt_dir, "config.json"), "w") as f:
            json.dump(cfg_json, f, indent=2)
        _save_st(os.path.join(ckpt_dir, "model.safetensors"), {n: store.master_view(n) for n in store.names})
        sync = diloco.sync.to(store.device) if diloco.sync.device != store.device else diloco.sync
        _save_st(os.path.join(ckpt_dir, "diloco_state.safetensors"),
                 {"theta_sync": sync, "outer_momentum": diloco.outer_optimizer.momentum_buffer,
                  **diloco.transport.shared_tensors()})
        state = {"step": step, "local_step": diloco.local_step, "outer_step_count": diloco.outer_step_count,
                 "outer_opt_step": diloco.outer_optimizer.step_count, "scheduler": diloco.scheduler.state_dict(),
                 "world_size": env.world_size, "inner_dp": env.inner_dp, "flat_numel": store.numel,
                 **shared, **(extra or {})}
        if inner_optimizer_kind(diloco.inner_optimizer) != "adamw":  # an AdamW checkpoint stays as it always was
            state["inner_optimizer"] = inner_optimizer_kind(diloco.inner_optimizer)
        with open(os.path.join(ckpt_dir, "trainer_state.json"), "w") as f:
            json.dump(state, f, indent=2)
    barrier(env)  # every rank's files are in the staging directory
    # every tensor above went through a host copy (so every collective it depends on has completed or been
    # aborted, and a watchdog abort sets the sticky error before it releases the collective): a failed own
    # RCCL communicator must not leave a COMPLETE checkpoint of partially reduced state behind
    for comm in (getattr(diloco, "outer_comm", None), getattr(diloco, "inner_comm", None)):
        if comm is not None:
            comm.check("the checkpoint is marked complete")
    if r == 0:
        with open(os.path.join(ckpt_dir, COMPLETE), "w") as f:
            json.dump({"step": step, "world_size": env.world_size}, f)
        _swap_in(ckpt_dir, final)
    barrier(env)


def load_checkpoint(ckpt_dir: str, model, diloco, env: DistEnv, elastic: bool = False) -> Dict[str, Any]:
    """``elastic`` (``--elastic-resume``): the number of DiLoCo workers may differ from the checkpoint's (one GPU
    per worker, a checkpoint without a pending overlapped outer step).  The shared outer state (theta_sync,
    outer momentum, schedule) is exact; worker r keeps its own AdamW state when the checkpoint has rank r, and a
    NEW worker starts from rank 0's AdamW state -- the "average over the survivors" recovery DiLoCo allows
    (SURVEY.md §5.3).  Data: the memmap stream is global (csrc/runtime/token_loader.cpp), so every worker
    restarts it where the old workers stopped together (``data_state_rank0``; nothing repeated or skipped);
    the HF loader's contiguous shards cannot be re-cut exactly and the resume refuses; synthetic workers keep
    their own random stream (new ones draw a fresh one).  Error-feedback residuals: surviving ranks keep their
    ``qef.send``, new workers and every ``qef.reduce`` start at zero (``QuantisedTransport.load_error_feedback_state``)."""
    found = find_checkpoint(ckpt_dir)
    if found is None:
        raise FileNotFoundError(f"no complete checkpoint at {ckpt_dir}")
    ckpt_dir = found
    with open(os.path.join(ckpt_dir, "trainer_state.json")) as f:
        state = json.load(f)
    store = model.store
    saved_opt, this_opt = state.get("inner_optimizer", "adamw"), inner_optimizer_kind(diloco.inner_optimizer)
    if saved_opt != this_opt:
        raise ValueError(f"checkpoint {ckpt_dir} was written with --inner-optimizer {saved_opt}, this run has "
                         f"{this_opt}: the optimizer state is not interchangeable, resume with the same optimizer")
    old_world = int(state.get("world_size", env.world_size))
    resized = elastic and old_world != env.world_size
    streamed = state.get("streaming")
    want = diloco.transport.shared_state()[0].get("streaming")  # this run's options, as a save would record them
    if streamed and elastic:
        raise ValueError(f"checkpoint {ckpt_dir} was written by a streaming run (per-worker local weights): "
                         f"--elastic-resume is not supported for it")
    if streamed and not want:
        raise ValueError(f"checkpoint {ckpt_dir} was written with --streaming-fragments {streamed['fragments']}: "
                         f"resume with the same streaming options")
    if want and not streamed:
        raise ValueError(f"checkpoint {ckpt_dir} was written without streaming: resume without "
                         f"--streaming-fragments")
    if want:
        for key in ("fragments", "pattern", "overlap", "alpha"):
            if streamed.get(key) != want[key]:
                raise ValueError(f"checkpoint {ckpt_dir} was written with streaming {key}={streamed.get(key)!r}, "
                                 f"this run has {want[key]!r}: resume needs the same streaming options")
    if resized:
        if env.inner_dp != 1 or int(state.get("inner_dp", 1)) != 1:
            raise ValueError("--elastic-resume needs one GPU per worker (--inner-dp 1) in both runs")
        if state.get("pending_outer"):
            raise ValueError(f"checkpoint {ckpt_dir} holds a pending overlapped outer step (per-worker state): "
                             f"--elastic-resume needs a checkpoint without one")
    # topology: every rank restores its OWN AdamW state and (two-level mode) its shard of the outer
    # step, so a resume on a different layout would silently drop workers' state or mis-shard the
    # outer momentum -- refuse it (unless --elastic-resume, above)
    for key, have in (("world_size", env.world_size), ("inner_dp", env.inner_dp), ("flat_numel", store.numel)):
        if key == "world_size" and resized:
            continue
        if key in state and int(state[key]) != int(have):
            raise ValueError(f"checkpoint {ckpt_dir} was written with {key}={state[key]}, this run has {have}: "
                             f"resume needs the same world size, --inner-dp and model (or --elastic-resume)")
    sd = _load_st(os.path.join(ckpt_dir, "model.safetensors"))
    model.load_state_dict(sd)
    ds = _load_st(os.path.join(ckpt_dir, "diloco_state.safetensors"))
    diloco.load_state_dict({"sync": ds["theta_sync"],
                            "outer": {"momentum_buffer": ds["outer_momentum"], "step": state["outer_opt_step"]},
                            "scheduler": state["scheduler"], "local_step": state["local_step"],
                            "outer_step_count": state["outer_step_count"]})
    rfile = os.path.join(ckpt_dir, f"rank{env.rank}.safetensors")
    data_state: Dict[str, Any] = {}
    own = os.path.exists(rfile)
    t_per, t_scal = {}, {}  # what the transport restores from: this rank's OWN files
    if not own and resized:  # a worker the checkpoint did not have: rank 0's AdamW state, fresh data stream
        rfile = os.path.join(ckpt_dir, "rank0.safetensors")
    elif not own and "world_size" in state:
        raise FileNotFoundError(f"{rfile} missing: the checkpoint is incomplete for rank {env.rank}")
    if os.path.exists(rfile):
        per = _load_st(rfile)
        diloco.inner_optimizer.exp_avg.copy_(per["adamw.exp_avg"])
        diloco.inner_optimizer.exp_avg_sq.copy_(per["adamw.exp_avg_sq"])
        with open(rfile[:-len(".safetensors")] + ".json") as f:
            scal = json.load(f)
        diloco.inner_optimizer.step_count = int(scal["adamw_step"])
        if own:
            t_per, t_scal = per, scal
            for k, v in per.items():
                if k.startswith("data."):
                    data_state[k[5:]] = v
            for k, v in scal.items():
                if k.startswith("data."):
                    data_state[k[5:]] = v
    shared_t = {k: v for k, v in ds.items() if k not in ("theta_sync", "outer_momentum")}  # transport.shared_tensors()
    for line in diloco.transport.load_state(t_per, t_scal, {**state, **shared_t}):
        print(f"[resume] rank {env.rank}: {line}", flush=True)
    state["data_state"] = data_state
    if resized:
        # the data sources whose stream is global (memmap) restart every worker -- survivors and new ones --
        # at the position the old workers reached together; they advance in lockstep, so rank 0's state says
        per0 = _load_st(os.path.join(ckpt_dir, "rank0.safetensors"))
        with open(os.path.join(ckpt_dir, "rank0.json")) as f:
            scal0 = json.load(f)
        ds0 = {k[5:]: v for k, v in list(per0.items()) + list(scal0.items()) if k.startswith("data.")}
        state["data_state_rank0"] = ds0
    state["resized_from"] = old_world if resized else None
    store.sync_shadow()
    return state
