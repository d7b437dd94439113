"""End-to-end HIP path vs the PyTorch reference path on the GPU (same weights, same batch)."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.optim import FlatAdamW

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    ops.set_backend("auto")


def _run(cfg, backend, ids, dtype, residual_dtype=None, fp8=False):
    ops.set_backend(backend)
    m = LlamaForCausalLM(cfg, "cuda", dtype, residual_dtype=residual_dtype, fp8=fp8).init_weights(3)
    out = m(ids, labels=ids)
    out.loss.backward()
    torch.cuda.synchronize()
    return out.loss.item(), m.store.grad.clone()


@pytest.mark.parametrize("kv", [4, 2])
def test_hip_vs_torch_model(kv):
    cfg = LlamaConfig.from_dict(dict(hidden_size=256, intermediate_size=512, num_attention_heads=4,
                                     num_key_value_heads=kv, num_hidden_layers=2, vocab_size=1000,
                                     rms_norm_eps=1e-5))
    ids = torch.randint(0, 1000, (2, 256), device="cuda")
    l_t, g_t = _run(cfg, "torch", ids, torch.float32)
    l_h, g_h = _run(cfg, "hip", ids, torch.bfloat16)
    assert abs(l_t - l_h) < 2e-2 * abs(l_t)
    rel = ((g_t - g_h).norm() / g_t.norm()).item()
    assert rel < 5e-2, rel


@pytest.mark.parametrize("fp8", [False, True])
def test_bf16_residual_model_tracks_fp32(fp8):
    """--residual-dtype bf16 (HIP, bf16 compute, optionally fp8 projections) against the fp32 torch model: the
    loss within the fp32-residual HIP model's tolerance, the gradient error at most a little above the
    fp32-residual HIP model's own error (fp8: ~0.1 relative to fp32 either way)."""
    cfg = LlamaConfig.from_dict(dict(hidden_size=256, intermediate_size=512, num_attention_heads=4,
                                     num_key_value_heads=2, num_hidden_layers=2, vocab_size=1000,
                                     rms_norm_eps=1e-5))
    ids = torch.randint(0, 1000, (2, 256), generator=torch.Generator().manual_seed(1)).cuda()
    l_t, g_t = _run(cfg, "torch", ids, torch.float32)
    rels = {}
    for rdt in (torch.float32, torch.bfloat16):
        l_h, g_h = _run(cfg, "hip", ids, torch.bfloat16, residual_dtype=rdt, fp8=fp8)
        assert abs(l_t - l_h) < 2e-2 * abs(l_t), (rdt, l_t, l_h)
        rels[rdt] = ((g_t - g_h).norm() / g_t.norm()).item()
    assert rels[torch.bfloat16] < 1.25 * rels[torch.float32] + 1e-2, rels
    if not fp8:
        assert rels[torch.bfloat16] < 5e-2, rels


@pytest.mark.parametrize("res", ["fp32", "bf16"])
def test_hip_vs_torch_loss_trajectory(res):
    """40 clip + AdamW steps on learnable data (every sequence follows one fixed random next-token
    permutation): the HIP bf16 model tracks the fp32 torch model's loss curve step by step, on fresh
    batches (not a memorised one), GQA 4/2; with the fp32 and the bf16 residual stream."""
    V = 512
    cfg = LlamaConfig.from_dict(dict(hidden_size=256, intermediate_size=512, num_attention_heads=4,
                                     num_key_value_heads=2, num_hidden_layers=2, vocab_size=V,
                                     rms_norm_eps=1e-5))
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(0))

    def batch(step):
        tok = torch.randint(0, V, (8,), generator=torch.Generator().manual_seed(100 + step))
        seq = [tok]
        for _ in range(255):
            seq.append(perm[seq[-1]])
        return torch.stack(seq, 1).cuda()

    curves = {}
    for backend, dt in (("torch", torch.float32), ("hip", torch.bfloat16)):
        ops.set_backend(backend)
        rdt = torch.bfloat16 if (backend == "hip" and res == "bf16") else None
        m = LlamaForCausalLM(cfg, "cuda", dt, residual_dtype=rdt).init_weights(3)
        opt = FlatAdamW(m.store, lr=1.5e-3)
        ls = []
        for step in range(40):
            ids = batch(step)
            out = m(ids, labels=ids)
            out.loss.backward()
            opt.step()
            m.store.zero_grad()
            ls.append(out.loss.item())
        curves[backend] = ls
    t, h = curves["torch"], curves["hip"]
    # 5-step means: single steps of a fast-learning run are chaotic in both precisions
    wt = [sum(t[i:i + 5]) / 5 for i in range(0, 40, 5)]
    wh = [sum(h[i:i + 5]) / 5 for i in range(0, 40, 5)]
    curve = " ".join(f"{a:.3f}/{b:.3f}" for a, b in zip(t, h))
    assert wt[-1] < 0.75 * t[0] and wh[-1] < 0.75 * h[0], curve
    assert max(abs(a - b) for a, b in zip(wt, wh)) < 0.04 * t[0], curve


def test_fp32_hip_path_runs():
    cfg = LlamaConfig.from_dict(dict(hidden_size=128, intermediate_size=256, num_attention_heads=4,
                                     num_hidden_layers=1, vocab_size=500, rms_norm_eps=1e-5))
    ops.set_backend("hip")
    m = LlamaForCausalLM(cfg, "cuda", torch.bfloat16).init_weights(0)
    opt = FlatAdamW(m.store, lr=1e-2)
    ids = torch.randint(0, 500, (4, 64), device="cuda")
    losses = []
    for _ in range(20):
        out = m(ids, labels=ids)
        out.loss.backward()
        opt.step()
        m.store.zero_grad()
        losses.append(out.loss.item())
    assert losses[-1] < losses[0] - 1.0, losses  # memorises a fixed batch


def test_smoke_entry():
    import __graft_entry__ as g
    g.smoke()


@pytest.mark.parametrize("rdt", [torch.float32, torch.bfloat16])
def test_hip_graph_matches_eager(rdt):
    """Captured micro-step replays == eager micro-steps (gradients accumulate in the flat buffer); fp32 and bf16
    residual streams."""
    from nanodiloco_amd.utils.graphs import GraphedMicroStep
    ops.set_backend("hip")
    cfg = LlamaConfig.from_dict(dict(hidden_size=256, intermediate_size=512, num_attention_heads=4,
                                     num_key_value_heads=2, num_hidden_layers=2, vocab_size=1000))
    batches = [torch.randint(0, 1000, (2, 256), device="cuda") for _ in range(5)]
    m1 = LlamaForCausalLM(cfg, "cuda", torch.bfloat16, residual_dtype=rdt).init_weights(3)
    losses1 = []
    for ids in batches:
        out = m1(ids, labels=ids, loss_scale=0.2)
        out.loss.backward()
        losses1.append(out.loss.item())
    m2 = LlamaForCausalLM(cfg, "cuda", torch.bfloat16, residual_dtype=rdt).init_weights(3)
    g = GraphedMicroStep(m2)
    losses2 = [g(ids, ids, 0.2).item() for ids in batches]  # 2 eager warm-ups, capture, 3 replays
    torch.cuda.synchronize()
    assert g.graph is not None
    for a, b in zip(losses1, losses2):
        assert abs(a - b) < 1e-4 * abs(a), (losses1, losses2)
    rel = ((m1.store.grad - m2.store.grad).norm() / m1.store.grad.norm()).item()
    assert rel < 1e-4, rel


def _trajectory(cfg, batches, graphed, seed=5):
    """Losses, the grad of the last accumulated micro-batch pair and the final weights of a few
    micro-batches with an optimizer step every second one."""
    from nanodiloco_amd.utils.graphs import GraphedMicroStep
    m = LlamaForCausalLM(cfg, "cuda", torch.bfloat16).init_weights(seed)
    opt = FlatAdamW(m.store, lr=1e-3)
    g = GraphedMicroStep(m) if graphed else None
    losses, grad = [], None
    for i, ids in enumerate(batches):
        if g is not None:
            losses.append(g(ids, ids, 0.5).clone())
        else:
            out = m(ids, labels=ids, loss_scale=0.5)
            out.loss.backward()
            losses.append(out.loss.detach())
        if i % 2 == 1:
            grad = m.store.grad.clone()
            opt.step()
            opt.zero_grad()
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), grad, m.store.master.clone()


def _rel(a, b):
    return ((a - b).float().norm() / b.float().norm()).item()


def _schedule_check(cfg, batches, graphed, switch, floor_g=1e-3, floor_p=1e-4, floor_l=2e-4):
    """Run the reference schedule twice (its own run-to-run spread: hipBLASLt stream-K GEMMs and the
    embedding's float atomics are not bitwise reproducible) and the switched schedule once; the
    switched run must sit within a small multiple of that spread."""
    switch(False)
    l0, g0, p0 = _trajectory(cfg, batches, graphed)
    l0b, g0b, p0b = _trajectory(cfg, batches, graphed)
    switch(True)
    try:
        l1, g1, p1 = _trajectory(cfg, batches, graphed)
    finally:
        switch(False)
    # floors at bf16-rounding level: a read of a half-written gradient moves the affected weights by
    # ~lr in a wrong direction (>= 1e-2 relative on them), far above these
    tol_g = max(4 * _rel(g0b, g0), floor_g)
    tol_p = max(4 * _rel(p0b, p0), floor_p)
    tol_l = max(4 * (l0b - l0).abs().max().item(), floor_l)
    assert (l1 - l0).abs().max().item() <= tol_l, (l0, l0b, l1)
    assert _rel(g1, g0) <= tol_g, (_rel(g1, g0), _rel(g0b, g0))
    assert _rel(p1, p0) <= tol_p, (_rel(p1, p0), _rel(p0b, p0))


_CFG_SMALL = dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2,
                  num_hidden_layers=3, vocab_size=1000)


@pytest.mark.parametrize("graphed", [False, True])
def test_wgrad_overlap_matches_serial(graphed):
    """Weight-gradient GEMMs on the side stream (fork/join; also inside a captured HIP graph) give
    the serial schedule's gradients and optimizer trajectory.  A missing join (a read of a
    half-written gradient) lands orders of magnitude outside the run-to-run spread."""
    ops.set_backend("hip")
    cfg = LlamaConfig.from_dict(_CFG_SMALL)
    batches = [torch.randint(0, 1000, (4, 256), device="cuda") for _ in range(6)]
    # bf16-ulp floors: hipBLASLt's stream-K GEMMs co-running with the side stream combine their
    # partial tiles in a timing-dependent order (1 bf16 ulp on some outputs -> ~1e-3 on grads);
    # serial runs reproduce bitwise.  A missing join is >= 1e-2.
    _schedule_check(cfg, batches, graphed, ops.set_wgrad_overlap, floor_g=5e-3, floor_p=5e-4, floor_l=1e-3)


@pytest.mark.parametrize("graphed", [False, True])
def test_dgrad_transposed_weights(graphed):
    """Input gradients through the W^T copies: every cached copy equals the CURRENT weights' transpose
    after optimizer steps (refreshed lazily in eager mode, and before every HIP-graph replay), and
    the trajectory matches the plain-layout dgrad within bf16 rounding (the NT and NN GEMM kernels
    round differently, so not within the run-to-run spread)."""
    from nanodiloco_amd.utils.graphs import GraphedMicroStep
    ops.set_backend("hip")
    cfg = LlamaConfig.from_dict(_CFG_SMALL)
    batches = [torch.randint(0, 1000, (4, 256), device="cuda") for _ in range(7)]
    prev = ops.dgrad_transposed_enabled()
    try:
        # the fused-epilogue GEMMs need the W^T copies (they are off without them), so compare the two
        # dgrad layouts with the fusions off in both runs: this test is about the layouts
        ops.set_fused_epilogues(rope=False, mlp=False)
        ops.set_dgrad_transposed(False)
        l0, g0, p0 = _trajectory(cfg, batches, graphed)
        ops.set_dgrad_transposed(True)
        l1, g1, p1 = _trajectory(cfg, batches, graphed)
        ops.set_fused_epilogues(rope=True, mlp=True)
        # freshness of the copies after 3 optimizer steps + one more micro-batch
        m = LlamaForCausalLM(cfg, "cuda", torch.bfloat16).init_weights(5)
        opt = FlatAdamW(m.store, lr=1e-3)
        g = GraphedMicroStep(m) if graphed else None
        for ids in batches:
            if g is not None:
                g(ids, ids, 0.5)
            else:
                m(ids, labels=ids, loss_scale=0.5).loss.backward()
            opt.step()
            opt.zero_grad()
        ids = batches[0]
        if g is not None:
            g(ids, ids, 0.5)
        else:
            m(ids, labels=ids, loss_scale=0.5).loss.backward()
        torch.cuda.synchronize()
        assert len(m.proj.wt_cache) == 4 * cfg.num_hidden_layers + 1
        for key, (wt, ver, w) in m.proj.wt_cache.items():
            assert ver == m.store.version, key
            assert torch.equal(wt, w.t()), key
    finally:
        ops.set_dgrad_transposed(prev)
        ops.set_fused_epilogues(rope=True, mlp=True)
    assert ((l1 - l0).abs() / l0.abs()).max().item() < 1e-3, (l0, l1)
    assert _rel(g1, g0) < 2e-2
    assert _rel(p1, p0) < 5e-4


@pytest.mark.parametrize("graphed", [False, True])
def test_fused_epilogue_trajectory(graphed):
    """7 optimizer steps with the fused RoPE / SwiGLU / SwiGLU-backward GEMM epilogues vs the unfused
    op chain: the fused path rounds once where the chain rounds twice (RoPE on the fp32 accumulator,
    d(act) never rounded to bf16), so the trajectories agree to bf16 rounding, not bitwise."""
    ops.set_backend("hip")
    cfg = LlamaConfig.from_dict(_CFG_SMALL)
    batches = [torch.randint(0, 1000, (4, 256), device="cuda") for _ in range(7)]
    try:
        ops.set_fused_epilogues(rope=False, mlp=False)
        l0, g0, p0 = _trajectory(cfg, batches, graphed)
        ops.set_fused_epilogues(rope=True, mlp=True)
        l1, g1, p1 = _trajectory(cfg, batches, graphed)
    finally:
        ops.set_fused_epilogues(rope=True, mlp=True)
    assert ((l1 - l0).abs() / l0.abs()).max().item() < 2e-3, (l0, l1)
    assert _rel(g1, g0) < 5e-2
    assert _rel(p1, p0) < 5e-3


def test_trainer_auto_hip_graph_small_model(tmp_path):
    """``--hip-graph auto`` (default) captures the micro-step for the reference's launch-bound 10M
    default model and trains through the CLI trainer (loss logged, finite, decreasing on a repeat)."""
    import json
    from nanodiloco_amd.main import parse_args
    from nanodiloco_amd.trainer import Trainer
    log = tmp_path / "log.jsonl"
    args = parse_args(["--llama-config-file", "configs/llama_default.json", "--batch-size", "16",
                       "--per-device-batch-size", "8", "--seq-length", "256", "--total-steps", "6",
                       "--inner-steps", "3", "--warmup-steps", "1", "--lr", "3e-3", "--wandb", "off",
                       "--log-file", str(log), "--log-every", "1"])
    t = Trainer(args)
    assert t.graphed is not None
    t.train()
    recs = [json.loads(l) for l in open(log)]
    losses = [r["loss"] for r in recs if "loss" in r]
    assert len(losses) >= 6 and all(l == l for l in losses)
    assert t.graphed.graph is not None
