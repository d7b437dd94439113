"""The HIP path of the whole model against the float64 model oracle, per parameter (tests/_model_oracle.py).

Every case runs three things on the same weights (``init_weights`` at one seed) and the same batches: the HIP model in
bf16 under the case's switches, the twin (the same model under ``ops.set_backend("torch")``, bf16, same residual
dtype: stock PyTorch ops, computed once per batch set and shared) and the oracle.  The rule is in
``_model_oracle.check_grads`` / ``check_loss``; a launcher spy states which kernels had to run and which must not,
so that a switch that stops selecting its kernel fails.  The bounds below that are not the project's margin of 8
were measured on the MI355X as docs/PARITY.md (model gradients) records: each case prints its figures before it
asserts.
"""

import importlib

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import _ext, fp8 as f8ops

from . import _model_oracle as mo

linops = importlib.import_module("nanodiloco_amd.ops.linear")  # ``ops.linear`` itself is the function

pytestmark = pytest.mark.gpu

DEV, BF16, SEED = "cuda", torch.bfloat16, 3

# cfg: model, B x T.  A: every fused bf16 and fp8 path is supported; B: hd 32, rep 4, V % 8 != 0, 576 tokens (no
# multiple of 128); C: hd 128 (no fused RoPE GEMM); D: tied embeddings
CFGS = {
    "A": (dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2, vocab_size=1000),
          2, 256),
    "B": (dict(hidden_size=128, intermediate_size=384, num_attention_heads=4, num_key_value_heads=1, vocab_size=515),
          3, 192),
    "C": (dict(hidden_size=256, intermediate_size=512, num_attention_heads=2, num_key_value_heads=2, head_dim=128,
               vocab_size=1000), 2, 128),
    "D": (dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=4, vocab_size=512,
               tie_word_embeddings=True), 2, 256),
    # the smallest shape found at which the library's plan groups the MLP's two weight gradients into one launch
    # (with split-K 2); at A .. D it predicts no win and keeps two launches
    "E": (dict(hidden_size=384, intermediate_size=1024, num_attention_heads=6, num_key_value_heads=2,
               vocab_size=1000), 2, 256),
}

MARGIN = 8.0  # the project's margin (tests/_oracle64.py); measured: no bf16 case needs more than 1.72
MARGINS = {}  # case family -> margin, for a family that needs more than 8 (none does)
# Projection clause.  The twin's own |beta_p| is 3.10e-3 at most over all cases (A/residual_bf16, post-attention norm
# weight); 4 x that is 1.24e-2, above the 1e-2 the clause has to stay under, and doubling B on A, C and D did not
# move it (2.97e-3 at most then: a property of bf16 arithmetic on these widths, not of the token count).  The bound is
# therefore the cap itself, 3.2 x the twin's largest; the HIP model's largest |beta_p| is 3.5e-3 (E/defaults).
BETA_BOUND = 1e-2
# Loss clause floor: 4 x the largest |l_twin - l64| over all cases (1.84e-4, A/graph); the HIP model's largest error
# is 2.2e-4 (C).
LOSS_FLOOR = 7.4e-4
# fp8: no PyTorch fp8 twin; the unit stays the bf16 twin, so the per-element margin is large (38.7 measured; by the
# convention of docs/PARITY.md twice that, rounded up to a power of two) and the clause that matters is
# ||g[p] - g64[p]|| / ||g64[p]|| per parameter kind: 2 x the measured worst over all fp8 cases and both steps, each
# below 0.5, so that a missing or a doubled term (relative error 1) fails.  |beta_p| and the loss likewise at 2 x.
FP8_MARGIN = 128.0
FP8_BETA_BOUND = 7.6e-2  # measured 3.76e-2 (keep_mlp, step 0, layer-0 input norm weight)
FP8_LOSS_ABS = 2.2e-3  # measured 1.1e-3 (keep_both step 1) at a loss of 6.9
FP8_REL = {  # measured worst in the comment of each line
    "lm_head.weight": 0.17, "model.embed_tokens.weight": 0.25, "model.norm.weight": 0.17,  # 0.081, 0.123, 0.085
    "model.layers.input_layernorm.weight": 0.29, "model.layers.post_attention_layernorm.weight": 0.28,  # 0.142, 0.137
    "model.layers.self_attn.q_proj.weight": 0.31, "model.layers.self_attn.k_proj.weight": 0.30,  # 0.155, 0.150
    "model.layers.self_attn.v_proj.weight": 0.27, "model.layers.self_attn.o_proj.weight": 0.24,  # 0.132, 0.116
    "model.layers.mlp.gate_proj.weight": 0.29, "model.layers.mlp.up_proj.weight": 0.29,  # 0.144, 0.141
    "model.layers.mlp.down_proj.weight": 0.27,  # 0.135
}
assert all(v < 0.5 for v in FP8_REL.values())

FUSED = ["nd_gemm_pp_rope", "nd_gemm_pp_swiglu", "nd_gemm_pp_dswiglu"]
UNFUSED = ["nd_rope_inplace", "nd_swiglu_fwd", "nd_swiglu_bwd"]
FUSED_F8 = ["nd_gemm_pp_rope_f8", "nd_gemm_pp_swiglu_f8", "nd_gemm_pp_dswiglu_f8", "nd_gemm_pp_swiglu_f8q",
            "nd_gemm_pp_dswiglu_f8q"]


def _config(name, layers=2):
    d, B, T = CFGS[name]
    return LlamaConfig.from_dict(dict(d, num_hidden_layers=layers, rms_norm_eps=1e-5)), B, T


def _rope_fuses(c):
    """The fused RoPE GEMM takes hd 32 / 64 and a q|k width that is a multiple of its 64-column tile
    (ops.linear.linear_rope_supported): A and D; not B (q|k = 5 x 32 = 160 columns) and not C (hd 128)."""
    return c.head_dim in (32, 64) and ((c.num_attention_heads + c.num_key_value_heads) * c.head_dim) % 64 == 0


@pytest.fixture(autouse=True)
def _switches(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    saved = dict(fused=ops.fused_epilogues(), dgrad_t=ops.dgrad_transposed_enabled(), group=ops.wgrad_group_enabled(),
                 overlap=dict(linops._OVERLAP, streams=None, pending=None, keep=None), proj=ops.proj_gemm(),
                 det=ops.deterministic(), keep=f8ops.fp8_keep_fused(), epi=f8ops._EPI["enabled"],
                 fq=f8ops._FUSED["enabled"], lm=f8ops.fp8_lm_head())
    try:
        yield
    finally:
        ops.set_backend("auto")
        ops.set_fused_epilogues(**saved["fused"])
        ops.set_dgrad_transposed(saved["dgrad_t"])
        ops.set_wgrad_group(saved["group"])
        ops.set_wgrad_overlap((1 if saved["overlap"]["fence"] else 2) if saved["overlap"]["enabled"] else 0)
        ops.set_proj_gemm(saved["proj"])
        ops.set_deterministic(saved["det"])
        f8ops.set_fp8_keep_fused({(False, False): "none", (True, False): "rope", (False, True): "mlp",
                                  (True, True): "both"}[(saved["keep"]["rope"], saved["keep"]["mlp"])])
        f8ops.set_fp8_fused_epilogues(saved["epi"])
        f8ops.set_fused_quant(saved["fq"])
        f8ops.set_fp8_lm_head(saved["lm"])


# ------------------------------------------------------------------------------------------ batches
def _batches(cfg, kind, n, seed=100):
    """``n`` micro-batches (ids, labels, attention_mask or None) of config ``cfg``, each with its own ids.  All
    labels carry a run of -100.  ``plain``; ``left`` / ``right``: B = 3 with 0, 5 and 11 pad tokens per row; ``doc``:
    two EOS per row, one of them the last key of a 64-key block.  On A the second micro-batch has a row whose
    targets are all ignored."""
    c, B, T = _config(cfg)
    if kind in ("left", "right"):
        B = 3
    out = []
    for i in range(n):
        g = torch.Generator().manual_seed(seed + 17 * i + ord(cfg))
        ids = torch.randint(3, c.vocab_size, (B, T), generator=g)
        mask = None
        if kind in ("left", "right"):
            mask = torch.ones(B, T, dtype=torch.long)
            for b, npad in enumerate([0, 5, 11]):
                if npad and kind == "left":
                    mask[b, :npad] = 0
                elif npad:
                    mask[b, T - npad:] = 0
            ids[mask == 0] = 2
        if kind == "doc":
            for b in range(B):
                ids[b, 63] = c.eos_token_id  # the next document starts on a 64-key block edge
                ids[b, 101 + 13 * b] = c.eos_token_id
        labels = ids.clone()
        for b in range(B):
            labels[b, 20 + 9 * b:20 + 9 * b + 12] = -100
        if mask is not None:
            labels[mask == 0] = -100
        if cfg == "A" and i == 1:
            labels[1] = -100
        out.append((ids.to(DEV), labels.to(DEV), mask.to(DEV) if mask is not None else None))
    return out


def _pattern(numel):
    """A known non-zero start of the gradient buffer (multiples of 2^-6 in [-2, 2] / 64: exact in fp32)."""
    return ((torch.arange(numel, device=DEV) % 5).float() - 2.0) * 2.0 ** -6


def _run(cfg, backend, batches, loss_scale=1.0, layers=2, prefill=False, graphed=False, model_kw=None):
    """Forward + backward of every micro-batch into one gradient buffer; (losses, {name: gradient}, model)."""
    c, _, _ = _config(cfg, layers)
    ops.set_backend(backend)
    m = LlamaForCausalLM(c, DEV, BF16, **(model_kw or {})).init_weights(SEED)
    if prefill:
        m.store.grad.copy_(_pattern(m.store.numel))
    losses = []
    if graphed:
        from nanodiloco_amd.utils.graphs import GraphedMicroStep
        step = GraphedMicroStep(m)
        for ids, labels, mask in batches:
            assert mask is None
            losses.append(step(ids, labels, loss_scale).clone())
        assert step.graph is not None and step.eager_fallbacks == 0
    else:
        for ids, labels, mask in batches:
            out = m(ids, labels=labels, attention_mask=mask, loss_scale=loss_scale)
            out.loss.backward()
            losses.append(out.loss.detach())
    torch.cuda.synchronize()
    grads = mo.model_grads(m)
    if prefill:
        pat = _pattern(m.store.numel)
        grads = {n: (g.double() - pat[slice(*m.store.range(n))].view(g.shape).double()) for n, g in grads.items()}
    return [float(l) for l in losses], grads, m


_REF = {}


def _reference(cfg, kind, n, loss_scale, rdt=None, doc=False):
    """The twin and the oracle of one batch set, computed once and shared (never modified)."""
    key = (cfg, kind, n, loss_scale, rdt, doc)
    if key not in _REF:
        batches = _batches(cfg, kind, n)
        kw = dict(residual_dtype=rdt, doc_mask=doc)
        l_twin, g_twin, m = _run(cfg, "torch", batches, loss_scale, model_kw=kw)
        l64, g64 = mo.grads64_sum(m, [(i, l, mo.key_start(k) if k is not None else None) for i, l, k in batches],
                                  loss_scale, doc_mask=doc)
        _REF[key] = dict(batches=batches, l_twin=l_twin, g_twin=g_twin, l64=[float(l) for l in l64], g64=g64)
    return _REF[key]


def _judge(case, losses, grads, ref, margin=None, beta_bound=None, floor=None):
    """Print the figures, then assert the three clauses."""
    margin = MARGINS.get(case.split("/")[1], MARGIN) if margin is None else margin
    report = {}
    err = None
    try:
        mo.check_grads(grads, ref["g64"], ref["g_twin"], margin, BETA_BOUND if beta_bound is None else beta_bound,
                       report, case)
    except AssertionError as e:
        err = e
    worst = max(report.items(), key=lambda kv: (kv[1]["margin"] != kv[1]["margin"], kv[1]["margin"]))
    wb = max(report.items(), key=lambda kv: kv[1]["beta"])
    wt = max(report.items(), key=lambda kv: kv[1]["beta_twin"])
    le = max(abs(a - b) for a, b in zip(losses, ref["l64"]))
    lt = max(abs(a - b) for a, b in zip(ref["l_twin"], ref["l64"]))
    print(f"[model-grads] {case}: margin {worst[1]['margin']:.2f} ({worst[0]}), |beta| {wb[1]['beta']:.2e} ({wb[0]}), "
          f"twin |beta| {wt[1]['beta_twin']:.2e} ({wt[0]}), loss err {le:.2e}, twin loss err {lt:.2e}")
    if err is not None:
        raise err
    for a, b, t in zip(losses, ref["l64"], ref["l_twin"]):
        mo.check_loss(a, b, t, margin, LOSS_FLOOR if floor is None else floor, case)


# ------------------------------------------------------------------------------------------ bf16 cases
def _set(fn, *a, **kw):
    return lambda: fn(*a, **kw)


def _expect_defaults(cfg):
    c, _, _ = _config(cfg)
    rope = _rope_fuses(c)
    return dict(ran=FUSED[1:] + ([FUSED[0]] if rope else [UNFUSED[0]]),
                never=UNFUSED[1:] + ([UNFUSED[0]] if rope else [FUSED[0]]) + ["nd_gemm_pp", "nd_gemm_w128"])


def _wgrad2_groups(cfg, B=None):
    """Whether the library's own plan groups the MLP's two weight gradients at this shape (it groups only where its
    cost model predicts a win over two launches, csrc/gemm_wgrad.hip nd_wgrad2_splits)."""
    c, B0, T = _config(cfg)
    d, F = c.hidden_size, c.intermediate_size
    return _ext.lib().nd_wgrad2_splits(d, F, 2 * F, d, (B or B0) * T) > 0


UNFUSED_EXPECT = dict(ran=UNFUSED, never=FUSED + ["nd_wgrad2_splits", "nd_wgrad2"])

# name: (setting, model kwargs, batch kind, micro-batches, loss scale, prefill, graphed, spy expectation or None)
BF16_CASES = {
    "defaults": (None, {}, "plain", 1, 1.0, False, False, "defaults"),
    "unfused": (_set(ops.set_fused_epilogues, rope=False, mlp=False), {}, "plain", 1, 1.0, False, False,
                UNFUSED_EXPECT),
    "dgrad_plain": (_set(ops.set_dgrad_transposed, False), {}, "plain", 1, 1.0, False, False, UNFUSED_EXPECT),
    "wgrad_ungrouped": (_set(ops.set_wgrad_group, False), {}, "plain", 1, 1.0, False, False,
                        dict(ran=FUSED[1:], never=["nd_wgrad2_splits", "nd_wgrad2"])),
    "overlap_off": (_set(ops.set_wgrad_overlap, 0), {}, "plain", 1, 1.0, False, False, "defaults"),
    "overlap_on": (_set(ops.set_wgrad_overlap, 1), {}, "plain", 1, 1.0, False, False, "defaults"),
    "proj_pp": (_set(ops.set_proj_gemm, "pp"), {}, "plain", 1, 1.0, False, False,
                dict(ran=["nd_gemm_pp"], never=["nd_gemm_w128"])),
    "proj_w128": (_set(ops.set_proj_gemm, "w128"), {}, "plain", 1, 1.0, False, False,
                  dict(ran=["nd_gemm_w128"], never=["nd_gemm_pp"])),
    "proj_short": (_set(ops.set_proj_gemm, "short"), {}, "plain", 1, 1.0, False, False,
                   dict(ran=["nd_gemm_pp"], never=["nd_gemm_w128"])),  # every K here is <= 1024
    "residual_bf16": (None, dict(residual_dtype=BF16), "plain", 1, 1.0, False, False, "defaults"),
    "checkpointing": (None, dict(activation_checkpointing=True), "plain", 1, 1.0, False, False, "defaults"),
    "deterministic": (_set(ops.set_deterministic, True), {}, "plain", 1, 1.0, False, False,
                      dict(ran=["nd_embedding_bwd_sorted"], at_least=1, never=["nd_embedding_bwd"])),
    "accumulate": (None, {}, "plain", 2, 0.5, True, False, "defaults"),
    "graph": (None, {}, "plain", 5, 0.2, False, True, "defaults"),
    "left_pad": (None, {}, "left", 1, 1.0, False, False, "defaults"),
    "right_pad": (None, {}, "right", 1, 1.0, False, False, "defaults"),
    "doc_mask": (None, dict(doc_mask=True), "doc", 1, 1.0, False, False,
                 dict(ran=["nd_attn_fwd_doc", "nd_attn_bwd_fused_doc"], never=["nd_attn_fwd_ks"])),
}
BF16_MATRIX = ([("A", n) for n in BF16_CASES] + [("B", n) for n in BF16_CASES if n != "graph"]
               + [(cfg, n) for cfg in "CD" for n in ("defaults", "unfused", "accumulate")]
               + [("E", n) for n in ("defaults", "wgrad_ungrouped", "accumulate")])


@pytest.mark.parametrize("cfg,name", BF16_MATRIX, ids=[f"{c}-{n}" for c, n in BF16_MATRIX])
def test_bf16_model_gradients(cfg, name):
    setting, kw, kind, n, ls, prefill, graphed, expect = BF16_CASES[name]
    c, _, _ = _config(cfg)
    L = c.num_hidden_layers
    ref = _reference(cfg, kind, n, ls, kw.get("residual_dtype"), kw.get("doc_mask", False))
    if setting is not None:
        setting()
    with mo.spying() as spy:
        losses, grads, m = _run(cfg, "hip", ref["batches"], ls, prefill=prefill, graphed=graphed, model_kw=kw)
    case = f"{cfg}/{name}"
    print(f"[model-grads] {case}: launchers {dict(sorted(spy.calls.items()))} refused {dict(spy.refused)}")
    assert linops.wgrad_outstanding() == (set(), []), case  # the backward joined every side-stream weight gradient
    _judge(case, losses, grads, ref)
    if expect == "defaults":
        expect = _expect_defaults(cfg)
    expect = dict(expect)
    B = ref["batches"][0][0].shape[0]
    if "nd_wgrad2" not in expect["never"] and name != "dgrad_plain":
        # grouping on and the fused MLP running: the plan is asked once per layer, and the grouped kernel runs
        # wherever the plan groups
        expect["ran"] = list(expect["ran"]) + ["nd_wgrad2_splits"]
        assert _wgrad2_groups(cfg, B) == (cfg == "E"), case
        key = "ran" if _wgrad2_groups(cfg, B) else "never"
        expect[key] = list(expect[key]) + ["nd_wgrad2"]
    spy.expect(ran=expect["ran"], at_least=expect.get("at_least", L), never=expect["never"], case=case)
    if name == "overlap_on":
        assert len(linops._OVERLAP["streams"]) >= 1  # the side stream exists: weight gradients did go there
    if c.tie_word_embeddings:
        assert "lm_head.weight" not in grads and "lm_head.weight" not in m.store.names
        parts = {}
        i, l, _ = ref["batches"][0]
        g = mo.grads64(m, i, l, ls, parts=parts)[1]["model.embed_tokens.weight"]
        # both uses matter: either part alone is far from the sum the parameter must hold
        assert mo.rel_norm(parts["embed"], g) > 0.05 and mo.rel_norm(parts["lm"], g) > 0.05


# ------------------------------------------------------------------------------------------ layer hook
@pytest.mark.parametrize("checkpointing", [False, True])
def test_layer_hook_sees_final_spans(checkpointing):
    """``layer_hook(i)`` fires once per layer, in the order L-1 .. 0, and what it reads of layer i's span of the flat
    gradient buffer is final: bitwise what the span holds after the backward (weight gradients on the side stream)."""
    L = 3
    batches = _batches("A", "plain", 1)
    ops.set_wgrad_overlap(1)
    ops.set_backend("hip")
    c, _, _ = _config("A", L)
    m = LlamaForCausalLM(c, DEV, BF16, activation_checkpointing=checkpointing).init_weights(SEED)
    fired, seen = [], {}

    def hook(i):
        a, b = m.store.span(f"model.layers.{i}.")
        fired.append(i)
        seen[i] = m.store.grad[a:b].clone()

    m.layer_hook = hook
    ids, labels, _ = batches[0]
    m(ids, labels=labels).loss.backward()
    torch.cuda.synchronize()
    assert fired == list(range(L - 1, -1, -1)), fired
    for i in range(L):
        a, b = m.store.span(f"model.layers.{i}.")
        final = m.store.grad[a:b]
        assert bool(final.any())
        assert torch.equal(seen[i].view(torch.int32), final.view(torch.int32)), f"layer {i}: span changed after hook"
    # and the hooked run computes what the run without hooks does
    _, g, _ = _run("A", "hip", batches, layers=L, model_kw=dict(activation_checkpointing=checkpointing))
    for n in m.store.names:
        assert mo.rel_norm(m.store.grad_view(n), g[n]) < 1e-2, n


# ------------------------------------------------------------------------------------------ fp8 cases
F8_PLAIN = ["nd_gemm_pp_f8"]
# name: (cfg, setting, fp8_wgrad, expectation)
FP8_CASES = {
    "defaults": ("A", None, True, dict(ran=FUSED_F8 + F8_PLAIN + ["nd_wgrad_f8", "nd_rmsnorm_fwd_q"],
                                       never=FUSED + UNFUSED)),
    "wgrad_bf16": ("A", None, False, dict(ran=FUSED_F8[:3] + F8_PLAIN + ["nd_wgrad"],
                                          never=FUSED + UNFUSED + FUSED_F8[3:] + ["nd_wgrad_f8"])),
    "keep_rope": ("A", _set(f8ops.set_fp8_keep_fused, "rope"), True,
                  dict(ran=FUSED[:1] + FUSED_F8[1:] + ["nd_wgrad_f8"], never=FUSED_F8[:1] + FUSED[1:] + UNFUSED)),
    "keep_mlp": ("A", _set(f8ops.set_fp8_keep_fused, "mlp"), True,
                 dict(ran=FUSED[1:] + FUSED_F8[:1] + ["nd_wgrad_f8"], never=FUSED_F8[1:] + FUSED[:1] + UNFUSED)),
    "keep_both": ("A", _set(f8ops.set_fp8_keep_fused, "both"), True,
                  dict(ran=FUSED + F8_PLAIN + ["nd_wgrad_f8"], never=FUSED_F8 + UNFUSED)),
    "epilogues_off": ("A", _set(f8ops.set_fp8_fused_epilogues, False), True,
                      dict(ran=F8_PLAIN + ["nd_rope_inplace", "nd_wgrad_f8"], never=FUSED_F8 + FUSED)),
    "fused_quant_off": ("A", _set(f8ops.set_fused_quant, False), True,
                        dict(ran=FUSED_F8[:3] + ["nd_fp8_cast", "nd_wgrad_f8"],
                             never=FUSED_F8[3:] + ["nd_rmsnorm_fwd_q", "nd_rmsnorm_bwd_q", "nd_swiglu_fwd_q",
                                                   "nd_swiglu_bwd_q", "nd_ce_fwd_bwd_q8"])),
    "lm_head_bf16": ("A", _set(f8ops.set_fp8_lm_head, False), True,
                     dict(ran=FUSED_F8 + ["nd_wgrad_f8", "nd_ce_fwd_bwd"], never=["nd_ce_fwd_bwd_q8"] + FUSED)),
    # V = 512 (a multiple of 128): the only config whose lm head runs in fp8, on the tied embedding table: no bf16
    # weight gradient is left.  (The CE kernel that writes e5m2 dlogits itself takes 8192 < V <= 32768 only.)
    "D_lm_head_fp8": ("D", None, True, dict(ran=FUSED_F8 + F8_PLAIN + ["nd_wgrad_f8"],
                                            never=FUSED + UNFUSED + ["nd_wgrad", "nd_ce_fwd_bwd_q8"])),
    # 576 tokens: the fp8 weight-gradient kernel (tokens % 128) and the quantising epilogues must refuse, the bf16
    # weight gradient takes over; q|k is 160 columns wide, so RoPE runs apart
    "B_fallback": ("B", None, True, dict(ran=FUSED_F8[1:3] + F8_PLAIN + ["nd_wgrad", "nd_rope_inplace"],
                                         never=["nd_wgrad_f8"] + FUSED_F8[:1] + FUSED_F8[3:] + FUSED)),
}


@pytest.mark.parametrize("name", sorted(FP8_CASES))
def test_fp8_model_gradients(name):
    """Two steps with zero grad between them, both checked: the first use of every slot takes current scaling, the
    second the delayed-scaling history."""
    cfg, setting, wgrad, expect = FP8_CASES[name]
    c, _, _ = _config(cfg)
    L = c.num_hidden_layers
    ref = [_reference(cfg, "plain", 1, 1.0), _reference_second(cfg)]
    if setting is not None:
        setting()
    ops.set_backend("hip")
    m = LlamaForCausalLM(c, DEV, BF16, fp8=True, fp8_wgrad=wgrad).init_weights(SEED)
    failures = []
    with mo.spying() as spy:
        for step, r in enumerate(ref):
            m.store.zero_grad()
            ids, labels, _ = r["batches"][0]
            out = m(ids, labels=labels)
            out.loss.backward()
            torch.cuda.synchronize()
            m.fp8.recipe.update()
            grads, loss = mo.model_grads(m), float(out.loss)
            case = f"{cfg}/fp8_{name}/step{step}"
            rels = {}
            for n, g in grads.items():
                kind = ".".join(p for p in n.split(".") if not p.isdigit())
                rels[kind] = max(rels.get(kind, 0.0), mo.rel_norm(g, r["g64"][n]))
            print(f"[model-grads] {case}: rel " + ", ".join(f"{k.replace('model.', '').replace('.weight', '')} "
                                                            f"{v:.3f}" for k, v in sorted(rels.items()))
                  + f"; loss {loss:.4f} vs {r['l64'][0]:.4f} (twin {r['l_twin'][0]:.4f})")
            for kind, v in rels.items():
                if not v <= FP8_REL[kind]:
                    failures.append(f"{case}: {kind}: relative error {v:.3f} > {FP8_REL[kind]}")
            if not abs(loss - r["l64"][0]) <= FP8_LOSS_ABS:
                failures.append(f"{case}: loss {loss} vs {r['l64'][0]}")
            try:
                _judge(case, [loss], grads, r, margin=FP8_MARGIN, beta_bound=FP8_BETA_BOUND, floor=float("inf"))
            except AssertionError as e:
                failures.append(str(e)[:2000])
    print(f"[model-grads] {cfg}/fp8_{name}: launchers {dict(sorted(spy.calls.items()))} refused {dict(spy.refused)}")
    assert not failures, "\n".join(failures)
    spy.expect(ran=expect["ran"], at_least=L, never=expect["never"], case=f"{cfg}/fp8_{name}")


def _reference_second(cfg):
    """The second fp8 step's batch (other ids), with its twin and oracle."""
    key = (cfg, "second")
    if key not in _REF:
        batches = _batches(cfg, "plain", 1, seed=200)
        l_twin, g_twin, m = _run(cfg, "torch", batches)
        l64, g64 = mo.grads64_sum(m, [(i, l, None) for i, l, _ in batches])
        _REF[key] = dict(batches=batches, l_twin=l_twin, g_twin=g_twin, l64=[float(l) for l in l64], g64=g64)
    return _REF[key]
