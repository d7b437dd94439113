"""The whole Llama model in float64, differentiable, and the per-parameter gradient rule built on it.

Plain PyTorch in float64, written from the math in the ``models/llama.py`` docstring and ``ops/reference.py``; it
calls no op of the project (the RoPE tables, the shift of the labels, the key start of a padded batch and the
document starts of a packed window are all computed here).  It runs on whatever device its inputs live on and reads
the weights the model computes with: the bf16 shadow for the seven projections and the lm head, the fp32 master for
the norms and the embedding gather.  ``tests/test_model_oracle_cpu.py`` checks it against the project's PyTorch path
and against HF in float64; ``tests/test_model_grads_gpu.py`` holds the HIP model against it, per parameter.

The rule (``check_grads``), for every parameter p, with the twin = the same model on stock PyTorch ops in the same
precision (it measures how far bf16 arithmetic alone lands from the oracle, never the code under test):
  per element  |g[p] - g64[p]| <= margin * max|g_twin[p] - g64[p]|          (``_oracle64.check`` with rel = 0)
  projection   |beta_p| <= bound,  beta_p = <g[p] - g64[p], g64[p]> / <g64[p], g64[p]>   (a 1-3 % scale error of a
               whole tensor, which the per-element clause cannot see)
and for the loss  |l - l64| <= max(margin * |l_twin - l64|, floor).  docs/PARITY.md has the measured figures.

``LauncherSpy`` counts the calls of every launcher of the kernel library, so that a case can state which kernels
must have run and which must not: a fused path that silently falls back fails instead of passing on the other kernels.
"""
import collections
import contextlib

import torch

from . import _oracle64

IGNORE = -100
PROJECTIONS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


# ------------------------------------------------------------------------------------------ inputs of the model
def rope_tables(T, hd, theta, scaling=None, device=None):
    """cos / sin [T, hd] as the model defines them: fp32 angles pos * inv_freq in the HF cat(freqs, freqs) layout
    (the tables are an input of the kernels, taken as given), widened to float64."""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.int64, device=device).float() / hd))
    if scaling:
        kind = scaling.get("rope_type", scaling.get("type", "default"))
        if kind == "linear":
            inv = inv / float(scaling["factor"])
        elif kind != "default":
            raise NotImplementedError(f"rope scaling {kind!r} is not part of the oracle")
    ang = torch.outer(torch.arange(T, dtype=torch.float32, device=device), inv)
    ang = torch.cat([ang, ang], dim=-1)
    return ang.cos().double(), ang.sin().double()


def key_start(attention_mask):
    """First real key per row of an HF attention_mask [B, T]: the pad count under left padding, 0 under right."""
    return (attention_mask.long().cumsum(1) == 0).sum(1)


def doc_starts(ids, eos):
    """[B, T]: the first token of each token's document in a packed window (a document ends with its EOS)."""
    B, T = ids.shape
    t = torch.arange(T, device=ids.device).expand(B, T)
    begins = torch.ones(B, T, dtype=torch.bool, device=ids.device)
    begins[:, 1:] = ids[:, :-1] == eos
    return torch.where(begins, t, torch.zeros_like(t)).cummax(dim=1).values


def _lm_name(c):
    return "model.embed_tokens.weight" if c.tie_word_embeddings else "lm_head.weight"


def weights64(m, device):
    """{key: float64 tensor on ``device``} of what ``m`` computes with.  Keys are the HF names, except that the
    embedding gather reads ``embed`` (fp32 master) and the lm head reads ``lm`` (bf16 shadow): two tensors, also when
    the weights are tied."""
    c, st = m.config, m.store
    P = {"embed": st.master_view("model.embed_tokens.weight"), "lm": st.shadow_view(_lm_name(c))}
    for n in st.names:
        if n in ("model.embed_tokens.weight", "lm_head.weight"):
            continue
        P[n] = st.shadow_view(n) if any(k in n for k in PROJECTIONS) else st.master_view(n)
    return {k: v.detach().to(device=device, dtype=torch.float64).clone() for k, v in P.items()}


# ------------------------------------------------------------------------------------------ the model
def _rotate(x, cos, sin):  # x [B, H, T, hd]; half-split rotation: element i pairs with i + hd/2
    h = x.shape[-1] // 2
    return x * cos + torch.cat([-x[..., h:], x[..., :h]], dim=-1) * sin


def _norm(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def logits64(c, P, ids, kstart=None, doc_start=None):
    """Logits [B, T, V] of config ``c`` on the weights ``P`` (``weights64``).  Query q attends to keys lo <= k <= q,
    lo = 0, ``kstart[b]`` or ``doc_start[b, q]``; a query with no key (a left-pad row) gets probabilities 0."""
    assert kstart is None or doc_start is None
    nh, nkv, hd, eps = c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.rms_norm_eps
    B, T = ids.shape
    dev = ids.device
    cos, sin = rope_tables(T, hd, c.rope_theta, c.rope_scaling, dev)
    t = torch.arange(T, device=dev)
    ok = (t[None, :] <= t[:, None])[None].expand(B, T, T).clone()
    if kstart is not None:
        ok &= t.view(1, 1, T) >= kstart.to(dev).long().view(B, 1, 1)
    if doc_start is not None:
        ok &= t.view(1, 1, T) >= doc_start.to(dev).long().view(B, T, 1)
    ok = ok[:, None]
    seen = ok.any(-1, keepdim=True)
    h = P["embed"][ids]
    for i in range(c.num_hidden_layers):
        p = f"model.layers.{i}."
        y = _norm(h, P[p + "input_layernorm.weight"], eps)
        q = (y @ P[p + "self_attn.q_proj.weight"].t()).view(B, T, nh, hd).transpose(1, 2)
        k = (y @ P[p + "self_attn.k_proj.weight"].t()).view(B, T, nkv, hd).transpose(1, 2)
        v = (y @ P[p + "self_attn.v_proj.weight"].t()).view(B, T, nkv, hd).transpose(1, 2)
        q, k = _rotate(q, cos, sin), _rotate(k, cos, sin)
        k, v = k.repeat_interleave(nh // nkv, dim=1), v.repeat_interleave(nh // nkv, dim=1)
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        s = torch.where(seen, s.masked_fill(~ok, float("-inf")), torch.zeros_like(s))
        a = (torch.softmax(s, dim=-1) * seen) @ v
        h = h + a.transpose(1, 2).reshape(B, T, nh * hd) @ P[p + "self_attn.o_proj.weight"].t()
        y = _norm(h, P[p + "post_attention_layernorm.weight"], eps)
        g, u = y @ P[p + "mlp.gate_proj.weight"].t(), y @ P[p + "mlp.up_proj.weight"].t()
        h = h + (g * torch.sigmoid(g) * u) @ P[p + "mlp.down_proj.weight"].t()
    return _norm(h, P["model.norm.weight"], eps) @ P["lm"].t()


def forward64(m, ids, kstart=None):
    """Logits [B, T, V] in float64 of model ``m`` on ``ids``, on the device of ``ids``."""
    with torch.no_grad():
        return logits64(m.config, weights64(m, ids.device), ids, kstart=kstart)


def loss64(logits, labels):
    """HF causal-LM loss: position t predicts labels[t + 1], -100 ignored, mean over the valid targets (0 when
    there is none)."""
    B, T, V = logits.shape
    tgt = torch.full_like(labels, IGNORE)
    tgt[:, :-1] = labels[:, 1:]
    tgt = tgt.reshape(-1)
    ok = tgt != IGNORE
    x = logits.reshape(-1, V)
    picked = x.gather(1, torch.where(ok, tgt, torch.zeros_like(tgt))[:, None])[:, 0]
    rows = (torch.logsumexp(x, dim=-1) - picked) * ok
    return rows.sum() / ok.sum().clamp_min(1)


def grads64(m, ids, labels, loss_scale=1.0, kstart=None, doc_mask=False, parts=None):
    """(loss, {HF parameter name: float64 gradient of loss_scale * loss}) by torch.autograd; q / k / v and gate / up
    are separate entries.  Tied weights: the gradients of the two uses are summed into the one parameter (``parts``,
    a dict, receives them apart as ``embed`` and ``lm``)."""
    c = m.config
    P = {k: v.requires_grad_(True) for k, v in weights64(m, ids.device).items()}
    ds = doc_starts(ids, c.eos_token_id) if doc_mask else None
    loss = loss64(logits64(c, P, ids, kstart=kstart, doc_start=ds), labels)
    keys = list(P)
    gs = dict(zip(keys, torch.autograd.grad(loss * loss_scale, [P[k] for k in keys])))
    out = {k: g for k, g in gs.items() if k not in ("embed", "lm")}
    if parts is not None:
        parts.update(embed=gs["embed"], lm=gs["lm"])
    if c.tie_word_embeddings:
        out["model.embed_tokens.weight"] = gs["embed"] + gs["lm"]
    else:
        out["model.embed_tokens.weight"], out["lm_head.weight"] = gs["embed"], gs["lm"]
    return loss.detach(), out


def grads64_sum(m, batches, loss_scale=1.0, doc_mask=False):
    """Accumulation / graph replays: ``batches`` is a list of (ids, labels, kstart or None); returns the list of
    losses and the sum of the gradients."""
    losses, total = [], None
    for ids, labels, ks in batches:
        l, g = grads64(m, ids, labels, loss_scale, kstart=ks, doc_mask=doc_mask)
        losses.append(l)
        total = g if total is None else {k: total[k] + g[k] for k in g}
    return losses, total


def model_grads(m):
    """{HF parameter name: clone of its span of the flat gradient buffer}."""
    return {n: m.store.grad_view(n).detach().clone() for n in m.store.names}


# ------------------------------------------------------------------------------------------ the rule
def beta(g, g64):
    """<g - g64, g64> / <g64, g64>: the relative error of g along g64 (0 for a zero reference)."""
    r = g64.double().reshape(-1)
    den = float(r @ r)
    return float((g.double().reshape(-1) - r) @ r) / den if den > 0 else 0.0


def rel_norm(g, g64):
    den = float(g64.double().norm())
    return float((g.double() - g64.double()).norm()) / den if den > 0 else float(g.double().norm())


def check_grads(g, g64, g_twin, margin, beta_bound, report=None, case=""):
    """Both clauses of the rule on every parameter; ``report`` collects, per parameter kind (the HF name without
    its layer number), the worst needed margin, |beta| and the twin's |beta|."""
    assert set(g) == set(g64) == set(g_twin), (sorted(g), sorted(g64))
    errors = []
    for n in sorted(g64):
        kind = ".".join(p for p in n.split(".") if not p.isdigit())
        b, bt = beta(g[n], g64[n]), beta(g_twin[n], g64[n])
        if report is not None:
            e = report.setdefault(kind, {"margin": 0.0, "beta": 0.0, "beta_twin": 0.0})
            r = _oracle64.excess_ratio(g[n], g64[n], g_twin[n], rel=0.0)
            e["margin"] = r if (r != r or r > e["margin"]) else e["margin"]
            e["beta"], e["beta_twin"] = max(e["beta"], abs(b)), max(e["beta_twin"], abs(bt))
        try:
            _oracle64.check(g[n], g64[n], g_twin[n], margin=margin, name=n, rel=0.0, note=case)
        except AssertionError as err:
            errors.append("per element: " + str(err))
        if not abs(b) <= beta_bound:
            errors.append(f"projection: {n} [{case}]: beta = {b:+.3e} outside +-{beta_bound:.1e} "
                          f"(the twin's: {bt:+.3e})")
    if errors:
        raise AssertionError(f"{len(errors)} violations of the gradient rule\n" + "\n".join(errors))


def check_loss(l, l64, l_twin, margin, floor, case=""):
    err, unit = abs(float(l) - float(l64)), abs(float(l_twin) - float(l64))
    assert err <= max(margin * unit, floor), (f"loss [{case}]: {float(l)!r} vs float64 {float(l64)!r}: error "
                                              f"{err:.3e} > max({margin} x twin error {unit:.3e}, floor {floor:.1e})")


# ------------------------------------------------------------------------------------------ launcher spy
class LauncherSpy:
    """A proxy of the loaded kernel library that counts the calls per launcher name: ``calls`` (every call) and
    ``refused`` (a launcher that answered hipErrorInvalidValue, i.e. did not take the shape and launched nothing;
    the plan / switch / version entry points return numbers of their own and are never counted as refusals)."""

    INVALID_VALUE = 1
    _NOT_LAUNCHERS = ("nd_version", "nd_env_reload", "nd_env_describe", "nd_attn_decode_split", "nd_mlp_coef_set")

    def __init__(self, lib):
        self._lib = lib
        self.calls = collections.Counter()
        self.refused = collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        launcher = not (name.endswith("_splits") or "_set" in name or name in self._NOT_LAUNCHERS)

        def counted(*args):
            self.calls[name] += 1
            rc = fn(*args)
            if launcher and rc == self.INVALID_VALUE:
                self.refused[name] += 1
            return rc

        return counted

    def ran(self, name):
        return self.calls[name] - self.refused[name]

    def expect(self, ran=(), at_least=1, never=(), case=""):
        few = {n: self.ran(n) for n in ran if self.ran(n) < at_least}
        extra = {n: self.ran(n) for n in never if self.ran(n)}
        assert not few and not extra, (f"[{case}] launchers that had to run >= {at_least} times: {few}; launchers "
                                       f"that must not run: {extra}; all calls: {dict(self.calls)}; refused: "
                                       f"{dict(self.refused)}")


@contextlib.contextmanager
def spying():
    """Route every op through a ``LauncherSpy`` (every op asks ``_ext.lib()`` for the library at launch time)."""
    from nanodiloco_amd.ops import _ext
    spy = LauncherSpy(_ext.lib())
    with _ext.using(spy):
        yield spy
