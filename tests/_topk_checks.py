"""Checks of the two top-k transport ops against the in-test oracle (tests/_topk_oracle.py), written once and run on
CPU (tests/test_topk_cpu.py: the PyTorch path) and on the GPU (tests/test_topk_gpu.py: the HIP kernels).  Every
comparison is bitwise.  Wire buffers are sentinel-filled with guard bytes around them (the padding bytes inside a
slot must keep the sentinel too); fp32 buffers carry guard elements.

One exception to "bitwise" is written down here: IEEE 754 leaves the sign and payload of a NaN that an operation
GENERATES (inf - inf, the residual of a sent inf) to the implementation, and x86 and the GPU choose differently.
``same_bits`` therefore accepts two NaNs at the same place as equal and compares every other element by its bits."""
import numpy as np
import torch

from nanodiloco_amd import ops

from . import _topk_oracle as to
from ._qcomm_checks import GUARD, SENT, f32_guards_intact, guarded_bytes, guarded_f32, guards_intact

SIZES = [to.CHUNK, to.CHUNK + 4095, 3 * to.CHUNK + 5, 5]
KS = [1, 7, 64, 256, 4096]
DTYPES = [torch.float32, torch.bfloat16]
KINDS = ["random", "equal", "straddle", "lsb", "zero", "denormal", "inf", "resid"]
LR, MU = 0.7, 0.9


def same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    g = got.detach().cpu().contiguous().numpy()
    gn, wn = np.isnan(g), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(g.view(np.int32)[~gn], want.view(np.int32)[~wn]))


def make_input(kind, n, k, seed):
    """(sync, master, e) as fp32 numpy arrays.  The crafted kinds use master = 0, so acc = sync + e exactly as
    built; "random" and "resid" have a random master as well."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    master = np.zeros(n, dtype=np.float32)
    e = np.zeros(n, dtype=np.float32)
    m0 = min(n, to.CHUNK)  # the crafted part is the first chunk; later chunks stay random
    sign = np.where(rng.integers(0, 2, m0) == 1, np.float32(-1), np.float32(1))
    if kind == "random":
        master = rng.standard_normal(n).astype(np.float32)
        v = v + master  # one rounding; the oracle takes sync - master as the ops do
    elif kind == "equal":  # equal magnitudes, mixed signs: the first k indices win
        v[:m0] = np.float32(0.5) * sign
    elif kind == "straddle":  # some larger values, then a tie group that the k-th place cuts through
        big = rng.permutation(m0)[:k // 2]
        tie = rng.permutation(m0)[:min(m0, k + 3)]
        v[:m0][tie] = np.float32(0.25) * sign[tie]
        v[:m0][big] = np.float32(1.0) + rng.random(big.size).astype(np.float32)
    elif kind == "lsb":  # keys that differ only in the lowest mantissa bit
        bits = np.uint32(0x3F800000) | rng.integers(0, 2, m0).astype(np.uint32)
        v[:m0] = bits.view(np.float32) * sign
    elif kind == "zero":  # an all-zero chunk (with both zeros): index order decides
        v[:m0] = np.float32(0.0) * sign
    elif kind == "denormal":
        v[:m0] = (rng.integers(0, 50, m0).astype(np.uint32)).view(np.float32) * sign
    elif kind == "inf":
        v[rng.integers(0, m0)] = np.float32("inf")
    elif kind == "resid":
        master = rng.standard_normal(n).astype(np.float32)
        v = v + master
        e = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    else:
        raise ValueError(kind)
    return v, master, e


def run_select(sync, master, e, k, vdt, dev):
    """ops.pseudograd_topk in guarded buffers -> (slot bytes as numpy uint8, the residual tensor).  The inputs must
    come back untouched and nothing outside the outputs may be written."""
    n = sync.size
    bf16 = vdt == torch.bfloat16
    sf, s = guarded_f32(torch.from_numpy(sync), dev)
    mf, m = guarded_f32(torch.from_numpy(master), dev)
    ef, r = guarded_f32(torch.from_numpy(e), dev)
    full, slot = guarded_bytes(to.slot_bytes(n, k, bf16), dev)
    assert ops.topk_slot_bytes(n, k, vdt) == to.slot_bytes(n, k, bf16) and slot.numel() % 16 == 0
    ops.pseudograd_topk(s, m, r, slot, k, vdt)
    assert guards_intact(full), "pseudograd_topk wrote outside its slot"
    assert f32_guards_intact(sf) and f32_guards_intact(mf) and f32_guards_intact(ef)
    assert np.array_equal(s.cpu().numpy().view(np.int32), sync.view(np.int32))
    assert np.array_equal(m.cpu().numpy().view(np.int32), master.view(np.int32))
    return slot.cpu().numpy(), r


def check_select(n, k, vdt, dev, kind, seed=0):
    """Slot bytes and residual equal the oracle's, bitwise."""
    bf16 = vdt == torch.bfloat16
    sync, master, e = make_input(kind, n, k, 1000 * n + 10 * k + seed)
    idx, val, new_e, acc = to.select(sync, master, e, k, bf16)
    got_slot, got_e = run_select(sync, master, e, k, vdt, dev)
    want = to.pack(idx, val, fill=SENT)
    bad = np.flatnonzero(got_slot != want)
    assert bad.size == 0, f"{kind} n={n} k={k} {vdt}: {bad.size} slot bytes differ, first at {bad[:4]}"
    assert same_bits(got_e, new_e), f"{kind} n={n} k={k} {vdt}: residual differs"
    m0 = min(n, to.CHUNK)
    kk = min(k, m0)
    if kind == "equal":
        assert idx[0, :kk].tolist() == list(range(kk))
    if kind == "zero":
        assert idx[0, :kk].tolist() == list(range(kk)) and not np.any(to.values_f32(val)[0])
    if kind == "inf":
        assert np.isinf(to.values_f32(val)[0]).sum() == 1 and int(np.isnan(new_e).sum()) == 1
    last = n - (idx.shape[0] - 1) * to.CHUNK
    if last < k:  # a chunk shorter than k: all of it is sent, the other entries are unused
        assert idx[-1, :last].tolist() == list(range(last)) and (idx[-1, last:] == to.NONE).all()
        assert not np.any(to.values_f32(val)[-1, last:])
    # what was sent plus what is still owed is acc: exact for fp32 values and for bf16 (acc - bf16(acc) is exact)
    if kind != "inf":
        with np.errstate(all="ignore"):
            assert np.array_equal(to.dense_sum([(idx, val)], n) + new_e, acc + np.float32(0))


def check_select_wrap(chunks, k, vdt, dev):
    """More chunks than the capped grid has workgroups: the input repeats three base chunks, so chunk c must equal
    the oracle's chunk c % 3 (a workgroup's second chunk differs from its first: the period does not divide the grid)."""
    bf16 = vdt == torch.bfloat16
    period = 3
    bs, bm, be = make_input("resid", period * to.CHUNK, k, 77 + k)
    idx, val, new_e, _ = to.select(bs, bm, be, k, bf16)
    reps = -(-chunks // period)
    tile = lambda a: np.ascontiguousarray(np.concatenate([a] * reps)[:chunks * (a.size // period)])
    got_slot, got_e = run_select(tile(bs), tile(bm), tile(be), k, vdt, dev)
    want = to.pack(tile(idx.reshape(-1)).reshape(chunks, k), tile(val.reshape(-1)).reshape(chunks, k), fill=SENT)
    assert np.array_equal(got_slot, want)
    assert same_bits(got_e, tile(new_e))


def fabricate(n, k, w, bf16, seed):
    """W workers' slots with overlapping indices, unused (0xFFFF) entries in every chunk and values the format
    holds exactly.  Returns [(idx, val)] and the gathered wire buffer (numpy uint8)."""
    rng = np.random.default_rng(seed)
    nch = to.nchunks(n)
    slots = []
    for r in range(w):
        idx = np.full((nch, k), to.NONE, dtype=np.uint16)
        val = np.zeros((nch, k), dtype=np.uint16 if bf16 else np.float32)
        for c in range(nch):
            m = min(to.CHUNK, n - c * to.CHUNK)
            # full and partly used; in the first chunk every worker sends something, so index 0 overlaps
            cnt = min(m, k) if (r + c) % 2 == 0 else int(rng.integers(0 if c else 1, min(m, k) + 1))
            sel = np.sort(rng.permutation(m)[:cnt])
            if cnt:
                sel[0] = 0  # every worker that sends anything sends index 0: a certain overlap
                sel = np.unique(sel)
            x = (rng.standard_normal(sel.size) * 1e-2).astype(np.float32)
            idx[c, :sel.size] = sel
            val[c, :sel.size] = to.bf16_bits(x) if bf16 else x
        slots.append((idx, val))
    return slots, np.concatenate([to.pack(i, v, fill=SENT) for i, v in slots])


def check_apply(n, k, w, vdt, dev, first, shadow, seed=0):
    """ops.outer_nesterov_topk == ops.outer_nesterov (on the GPU: nd_outer_nesterov) fed with the oracle's
    worker-order sum, bitwise: master, sync, momentum and the bf16 shadow; nothing outside [0, n) is touched."""
    bf16 = vdt == torch.bfloat16
    slots, wire = fabricate(n, k, w, bf16, 31 * n + 7 * k + w + seed)
    dsum = torch.from_numpy(to.dense_sum(slots, n)).to(dev)
    if w > 1 and min(n, to.CHUNK) > 1:
        assert sum(int((i[0] == 0).any()) for i, _ in slots) > 1, "the fabricated slots must overlap"
    gfull, gath = guarded_bytes(wire.size, dev)
    gath.copy_(torch.from_numpy(wire))
    before = gfull.clone()
    g = torch.Generator().manual_seed(n + 3)
    m0, s0, b0 = (torch.randn(n, generator=g) for _ in range(3))

    def state():
        out = [guarded_f32(t, dev) for t in (m0, s0, b0)]
        out.append(guarded_f32(torch.zeros(n, dtype=torch.bfloat16), dev) if shadow else (None, None))
        return out

    (mf, m), (sf, s), (bf, b), (hf, h) = state()
    (mf2, m2), (sf2, s2), (bf2, b2), (hf2, h2) = state()
    inv_w = 1.0 / w
    ops.outer_nesterov_topk(m, s, gath, w, k, vdt, b, h, inv_w, LR, MU, first)
    ops.outer_nesterov(m2, s2, dsum, b2, h2, inv_w, LR, MU, first)
    assert torch.equal(gfull, before), "outer_nesterov_topk wrote to the wire buffer"
    for got, want in ((mf, mf2), (sf, sf2), (bf, bf2)):
        assert torch.equal(got, want)  # guards included: both leave them alone
        assert f32_guards_intact(got)
    assert not torch.equal(m, m0.to(dev)) and torch.equal(m, s)
    if shadow:
        assert torch.equal(hf, hf2) and f32_guards_intact(hf)
        assert torch.equal(h, m.to(torch.bfloat16))
    # and densify(), the helper the CPU path and the tools use, gives the oracle's sum
    assert torch.equal(ops.densify(gath, w, n, k, vdt), dsum)


def check_degenerate(m, dl, m2, dl2, steps=2):
    """k = 4096 with fp32 values sends everything: after ``steps`` outer steps master, sync and momentum equal the
    dense fp32 transport's (``m2`` / ``dl2``) as floats -- a -0.0 can become +0.0 through ``+ e`` -- and the
    residual is all zero."""
    st, st2 = m.store, m2.store
    assert torch.equal(st.master, st2.master)
    start = st.master.clone()
    for s in range(steps):
        drift = (0.01 * torch.randn(st.numel, generator=torch.Generator().manual_seed(50 + s))).to(st.master.device)
        for store, d in ((st, dl), (st2, dl2)):
            store.master.add_(drift)
            d.outer_step()
        assert torch.equal(st.master, st2.master) and torch.equal(dl.sync, dl2.sync)
        assert torch.equal(dl.outer_optimizer.momentum_buffer, dl2.outer_optimizer.momentum_buffer)
        assert torch.equal(st.shadow, st2.shadow)
        assert not bool(dl.topk_residual.any())
    assert not torch.equal(st.master, start)


def check_conservation(n, k, vdt, dev, steps=4):
    """Integer-valued pseudo-gradients with |v| <= 256: every fp32 add is exact and bf16 holds each entry or
    rounds it to another integer, so over ``steps`` steps the sum of everything sent plus the final residual
    equals the sum of the pseudo-gradients exactly, element by element."""
    rng = np.random.default_rng(n + k)
    resid = torch.zeros(n, device=dev)
    master = torch.zeros(n, device=dev)
    sent = torch.zeros(n, device=dev)
    total = np.zeros(n, dtype=np.float32)
    slot = torch.zeros(ops.topk_slot_bytes(n, k, vdt), dtype=torch.uint8, device=dev)
    for _ in range(steps):
        v = rng.integers(-256, 257, n).astype(np.float32)
        total += v
        ops.pseudograd_topk(torch.from_numpy(v).to(dev), master, resid, slot, k, vdt)
        sent += ops.densify(slot, 1, n, k, vdt)
    assert np.array_equal((sent + resid).cpu().numpy(), total)
    if k < min(n, to.CHUNK):
        assert bool((resid != 0).any()), "with k below the chunk length something must still be owed"
