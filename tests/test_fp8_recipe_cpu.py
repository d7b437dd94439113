"""The delayed-scaling bookkeeping of ``ops/fp8.py`` (``Fp8Recipe``) on the CPU device: ``update()`` is plain torch,
so the amax partials a quantiser kernel would have written are written by hand here.  No GPU needed."""
import pytest
import torch

from nanodiloco_amd.ops import fp8

FMTS = [fp8.E4M3, fp8.E5M2]


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _recipe(history=4, margin=1, capacity=6):
    r = fp8.Fp8Recipe("cpu", history=history, margin=margin, capacity=capacity)
    assert r.amax.shape == (capacity, fp8.AMAX_PARTS) and r.hist.shape == (capacity, history)
    return r


def expected_scale(fmt, amax, margin):
    """fmax / (amax * 2^margin) in fp32, as update() computes it."""
    return f32(fp8.FMAX[fmt]) / (f32(amax) * f32(2.0 ** margin))


@pytest.mark.parametrize("margin", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
def test_scale_is_fmax_over_the_history_maximum(fmt, margin):
    r = _recipe(history=4, margin=margin)
    k = r.new_slot(fmt)
    assert k == 0 and r.n == 1 and r.fmax[k].item() == fp8.FMAX[fmt]
    seen = []
    for step, a in enumerate([3.0, 0.75, 11.5, 0.125, 0.5, 0.25, 0.0625, 2.0]):
        # the maximum sits in a different partial slot every step; the other partials hold smaller values
        r.amax[k].fill_(a / 4)
        r.amax[k, (17 * step) % fp8.AMAX_PARTS] = a
        r.update()
        seen.append(a)
        m = max(seen[-4:])  # the last H = 4 amaxes
        assert r.scale[k].item() == expected_scale(fmt, m, margin).item(), (step, a, m)
        assert r.inv[k].item() == (1.0 / r.scale[k]).item()
        assert r.inv[k].item() == (f32(1.0) / expected_scale(fmt, m, margin)).item()
        assert bool((r.amax[k] == 0).all())  # the partials are cleared for the next step
    assert r.pos == 8 % 4


@pytest.mark.parametrize("H", [1, 3, 16])
def test_an_old_maximum_leaves_the_ring_after_exactly_H_updates(H):
    r = _recipe(history=H, margin=0)
    k = r.new_slot(fp8.E4M3)
    r.amax[k, 5] = 100.0
    r.update()
    big = expected_scale(fp8.E4M3, 100.0, 0).item()
    assert r.scale[k].item() == big
    for i in range(1, H + 1):
        r.amax[k, 0] = 1.0
        r.update()
        want = big if i < H else expected_scale(fp8.E4M3, 1.0, 0).item()  # the H-th later update overwrites it
        assert r.scale[k].item() == want, (H, i)


def test_a_slot_that_only_saw_zero_keeps_its_scale_and_others_are_untouched():
    r = _recipe(history=2, margin=1, capacity=6)
    k0, k1, k2 = r.new_slot(fp8.E4M3), r.new_slot(fp8.E5M2), r.new_slot(fp8.E4M3)
    r.scale[k1] = 23.0
    r.inv[k1] = 1.0 / 23.0
    # slots at index >= n: scale, inverse, partials and history stay as they are
    r.scale[3:] = 7.0
    r.inv[3:] = 0.25
    r.amax[3:] = 5.0
    r.hist[3:] = 9.0
    r.amax[k0, 63] = 2.0
    r.amax[k2, 0] = 4.0
    for _ in range(3):  # more updates than the ring is long
        r.update()
        assert r.scale[k1].item() == 23.0 and r.inv[k1].item() == (1.0 / f32(23.0)).item()
        assert bool((r.scale[3:] == 7.0).all()) and bool((r.inv[3:] == 0.25).all())
        assert bool((r.amax[3:] == 5.0).all()) and bool((r.hist[3:] == 9.0).all())
        assert bool((r.amax[:3] == 0).all())
    # k0 / k2 saw a value once; after it left the ring (H = 2) their history is all zero and the scale stays
    assert r.scale[k0].item() == expected_scale(fp8.E4M3, 2.0, 1).item()
    assert r.scale[k2].item() == expected_scale(fp8.E4M3, 4.0, 1).item()
    assert bool((r.hist[:3] == 0).all())
    assert torch.isfinite(r.scale).all() and torch.isfinite(r.inv).all()


def test_update_without_slots_is_a_no_op():
    r = _recipe()
    r.amax.fill_(3.0)
    r.update()
    assert r.pos == 0 and bool((r.amax == 3.0).all()) and bool((r.scale == 1.0).all())


def test_target_needs_a_ready_slot_and_fused_quantisation():
    r = _recipe()
    k = r.new_slot(fp8.E5M2)
    assert r.target(k, fp8.E5M2) is None  # first use is scaled from the tensor's own amax: only the cast can
    r.ready[k] = True
    t = r.target(k, fp8.E5M2)
    assert isinstance(t, fp8.QuantTarget) and (t.recipe, t.k, t.fmt, t.out) == (r, k, fp8.E5M2, None)
    q = t.alloc((2, 8), "cpu")
    assert q.dtype == torch.float8_e5m2 and q.shape == (2, 8)
    qp, sp, ap, parts, fmt = t.args(q)
    assert qp == q.data_ptr() and sp == r.scale[k:k + 1].data_ptr() and ap == r.amax[k].data_ptr()
    assert parts == fp8.AMAX_PARTS and fmt == fp8.E5M2
    fp8.set_fused_quant(False)
    try:
        assert r.target(k, fp8.E5M2) is None
    finally:
        fp8.set_fused_quant(True)
    assert r.target(k, fp8.E5M2) is not None


def test_take_stashed_matches_storage_and_shape_and_always_pops():
    r = _recipe()
    k = r.new_slot(fp8.E5M2)
    r.ready[k] = True
    g = torch.zeros(4, 8, dtype=torch.bfloat16)
    q = torch.zeros(4, 8, dtype=torch.uint8)
    assert r.take_stashed(k, g) is None  # nothing stashed
    r.target(k, fp8.E5M2).stash(g, q)
    assert r.take_stashed(k, g) is q
    assert k not in r.stash and r.take_stashed(k, g) is None  # popped
    # another tensor (other storage): no copy, and the entry is gone all the same
    r.target(k, fp8.E5M2).stash(g, q)
    assert r.take_stashed(k, g.clone()) is None
    assert k not in r.stash and r.take_stashed(k, g) is None
    # same storage pointer, other shape
    r.target(k, fp8.E5M2).stash(g, q)
    assert r.take_stashed(k, g.view(8, 4)) is None
    assert k not in r.stash
    # another slot's stash is not touched
    k2 = r.new_slot(fp8.E5M2)
    r.stash[k2] = (g.data_ptr(), q)
    assert r.take_stashed(k, g) is None and r.take_stashed(k2, g) is q
