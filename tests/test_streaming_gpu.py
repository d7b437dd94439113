"""HIP kernels of the Streaming DiLoCo fragment step (csrc/stream_outer.hip): ``nd_frag_pseudograd`` and
``nd_frag_outer_mix`` against torch on the packed slices and against the contiguous ``nd_outer_nesterov`` run span
by span (bitwise at alpha = 0), the alpha merge against an fp64 evaluation (one fp32 ulp), untouched gaps, and a
one-process ``Diloco`` round on the HIP path against the torch backend on the same device.

Grid cap: both kernels grid-stride 4 elements per lane over at most 2048 blocks of 256 lanes (the cap of
``optim.hip``'s vector streams, not the 4096 of ``nd_outer_nesterov``), so the ``big`` table is one 64-element chunk
past a full pass of THAT grid: 2048 * 256 * 4 + 64 elements."""
import os

import pytest
import torch

from nanodiloco_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = 2048 * 256 * 4 + 64


def _table(lengths, gap=64, lead=64):
    spans, a = [], lead
    for n in lengths:
        spans.append((a, a + n))
        a += n + gap
    return spans, a  # the flat size leaves a gap after the last span too


TABLES = {
    "one64": ([(0, 64)], 192),                 # one span of 64 at the very start
    "three": _table([64, 192, 64]),            # gaps between the spans
    "x33": _table([64] * 33),                  # crosses any block-to-span lookup boundary
    "big": _table([BIG]),                      # one vector chunk past a full pass of the capped grid
}
LR, MU, INV_W = 0.7, 0.9, 0.25


@pytest.fixture(autouse=True)
def _gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_INPUTS = {}


def _inputs(name):
    """Seeded buffers of one table, computed once and never modified (tests clone): the gaps carry the same
    random sentinel pattern as the spans."""
    if name not in _INPUTS:
        spans, n = TABLES[name]
        g = torch.Generator(device=DEV).manual_seed(len(spans) * 7919 + n)
        sync = torch.randn(n, device=DEV, generator=g)
        master = sync + 0.01 * torch.randn(n, device=DEV, generator=g)
        mom = 0.02 * torch.randn(n, device=DEV, generator=g)
        total = sum(b - a for a, b in spans)
        dsum = 0.04 * torch.randn(total, device=DEV, generator=g)
        shadow = torch.randn(n, device=DEV, generator=g).bfloat16()
        _INPUTS[name] = (spans, n, total, sync, master, mom, dsum, shadow)
    return _INPUTS[name]


def _gap_mask(spans, n):
    m = torch.ones(n, dtype=torch.bool, device=DEV)
    for a, b in spans:
        m[a:b] = False
    return m


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("name", list(TABLES))
def test_frag_pseudograd_bitwise(name):
    spans, n, total, sync, master, _, _, _ = _inputs(name)
    want = torch.cat([sync[a:b] - master[a:b] for a, b in spans])
    for dt in (torch.float32, torch.bfloat16):
        out = torch.full((total + 64,), 7.0, dtype=dt, device=DEV)  # 64 guard elements behind the packed end
        ops.frag_pseudograd(sync, master, ops.SpanTable(spans, DEV), out)
        assert _same(out[:total], want.to(dt))
        assert bool((out[total:] == 7.0).all())


def _run_mix(name, wire, sep_shadow, first, alpha):
    spans, n, total, sync, master, mom, dsum, shadow = _inputs(name)
    d = dsum.to(wire)
    got = [master.clone(), sync.clone(), mom.clone(), shadow.clone()]
    ops.frag_outer_mix(got[0], got[1], d, got[2], got[3] if sep_shadow else got[0], ops.SpanTable(spans, DEV), INV_W,
                       LR, MU, first, alpha)
    ref = [master.clone(), sync.clone(), mom.clone(), shadow.clone()]
    o = 0
    for a, b in spans:  # the contiguous kernel, span by span, on the matching packed slice
        ops.outer_nesterov(ref[0][a:b], ref[1][a:b], d[o:o + b - a], ref[2][a:b],
                           ref[3][a:b] if sep_shadow else None, INV_W, LR, MU, first)
        o += b - a
    gap = _gap_mask(spans, n)
    for x, orig in zip(got, (master, sync, mom, shadow)):  # outside the spans nothing is written
        assert _same(x[gap], orig[gap])
    return got, ref, master, gap


@pytest.mark.parametrize("sep_shadow", [True, False], ids=["bf16shadow", "aliased"])
@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16], ids=["f32wire", "bf16wire"])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("name", list(TABLES))
def test_frag_outer_mix_alpha0_is_bitwise_outer_nesterov(name, first, wire, sep_shadow):
    got, ref, _, _ = _run_mix(name, wire, sep_shadow, first, 0.0)
    for x, y, what in zip(got, ref, ("master", "sync", "momentum", "shadow")):
        assert _same(x, y), what
    if not sep_shadow:  # an aliased shadow is never written as bf16
        assert _same(got[3], _inputs(name)[7])


@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16], ids=["f32wire", "bf16wire"])
@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("name", list(TABLES))
def test_frag_outer_mix_alpha_one_ulp(name, alpha, wire):
    got, ref, p0, gap = _run_mix(name, wire, True, False, alpha)
    assert _same(got[1], ref[1]) and _same(got[2], ref[2])             # sync, momentum: as at alpha = 0
    inside = ~gap
    th = got[1][inside]
    x = p0[inside] - th                                                 # fp32, as the kernel forms it
    want = th.double() + alpha * x.double()
    err = (got[0][inside].double() - want).abs()
    print(f"{name} alpha={alpha}: max err / (2^-23 |v|) = {(err / (2.0 ** -23 * want.abs())).max().item():.3f}")
    assert bool((err <= 2.0 ** -23 * want.abs()).all())
    assert _same(got[3][inside], got[0][inside].bfloat16())             # shadow == bf16(master)
    assert not _same(got[0][inside], th)                                # the merge did something


def test_span_table_refused_before_launch():
    x = torch.zeros(512, device=DEV)
    for bad in ([(0, 100)], [(32, 96)], [(0, 128), (64, 192)], [(448, 576)]):
        with pytest.raises(ValueError):
            ops.frag_pseudograd(x, x, bad, torch.zeros(512, device=DEV))
        with pytest.raises(ValueError):
            ops.frag_outer_mix(x, x.clone(), torch.zeros(512, device=DEV), x.clone(), None, bad, 1.0, LR, MU, True)


# ------------------------------------------------------------------ one-process Diloco: HIP path vs torch backend
def _round(alpha, backend):
    from nanodiloco_amd.config import LlamaConfig
    from nanodiloco_amd.models import LlamaForCausalLM
    from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
    from nanodiloco_amd.parallel.diloco import Diloco
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    prev = ops.get_backend()
    ops.set_backend(backend)
    try:
        cfg = LlamaConfig.from_dict(dict(hidden_size=32, intermediate_size=64, num_attention_heads=2,
                                         num_hidden_layers=4, vocab_size=50, rms_norm_eps=1e-5))
        m = LlamaForCausalLM(cfg, torch.device(DEV), torch.bfloat16).init_weights(11)
        st = m.store
        assert st.shadow.data_ptr() != st.master.data_ptr()
        H = 8
        dl = Diloco(m, FlatAdamW(st, lr=1e-3), FlatOuterNesterov(st, lr=LR, momentum=MU), 2, 2 * H, H,
                    fragments=2, stream_overlap=1, stream_alpha=alpha)
        g = torch.Generator(device=DEV).manual_seed(5)
        events = []
        for t in range(1, H + 2):  # sends after 4 and 8, applies after 5 and 9
            st.master.add_(0.01 * torch.randn(st.numel, device=DEV, generator=g))
            ev = dl.stream_step(t)
            if ev:
                events.append((t, ev["sent"], ev["applied"]))
        assert events == [(4, 0, None), (5, None, 0), (8, 1, None), (9, None, 1)]
        assert dl.outer_step_count == 1 and st.version >= 2
        return [x.clone() for x in (st.master, dl.sync, dl.outer_optimizer.momentum_buffer, st.shadow)], \
            dl.frag_tables[1].spans
    finally:
        ops.set_backend(prev)


@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_diloco_round_hip_vs_torch_backend(alpha):
    (hip, last), (ref, _) = _round(alpha, "auto"), _round(alpha, "torch")
    assert not _same(hip[1], torch.zeros_like(hip[1]))
    if alpha == 0.0:
        for x, y, what in zip(hip, ref, ("master", "sync", "momentum", "shadow")):
            assert _same(x, y), what
        return
    assert _same(hip[1], ref[1]) and _same(hip[2], ref[2])
    err = (hip[0].double() - ref[0].double()).abs()
    assert bool((err <= 2.0 ** -23 * ref[0].double().abs()).all())
    sh = (hip[3].float() - ref[3].float()).abs()  # the shadows round masters at most one fp32 ulp apart
    assert bool((sh <= 2.0 ** -7 * ref[3].float().abs()).all())
    for a, b in last:  # the fragment applied last (the test's drift bypasses the shadow of the other one)
        assert _same(hip[3][a:b], hip[0][a:b].bfloat16())
