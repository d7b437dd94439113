"""Checks of the four low-rank transport ops (ops/lowrank_comm.py) against the float64 oracle of
tests/_lowrank_oracle.py, written once and run on the CPU (tests/test_lowrank_cpu.py: the PyTorch path) and on the GPU
(tests/test_lowrank_gpu.py: the HIP kernels).  Every fp32 buffer carries guard elements; tensors sit at 64-aligned
offsets of a flat buffer, so there are gaps that no table row covers and nothing may touch.

Each check returns the largest ``error / bound`` it saw (the margin docs/DESIGN.md records)."""
import numpy as np
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops.lowrank_comm import LowRankPlan

from . import _lowrank_oracle as lo
from ._qcomm_checks import f32_guards_intact, guarded_f32

LR, MU = 0.7, 0.9
GRID_CAP = 1024  # csrc/lowrank_comm.hip: every kernel strides over the work past this many workgroups
# rank, tensors in flat order (1-D: a dense span of that length)
CASES = {
    "r16": (16, [(64, 64), (1,), (63, 64), (5,), (64, 80)]),      # exactly min = 4R; 63 x 64 is below the rule
    "r8": (8, [(257, 72), (1,), (72, 260), (5,)]),                # m odd, n no multiple of the 64- / 256-column blocks
    "r1": (1, [(1000, 128), (5,), (36, 8)]),                      # embedding-like, m >> n
    "r32": (32, [(1000, 128), (1,), (128, 1000)]),
    "r4": (4, [(66, 70), (40, 16), (5,), (20, 24)]),              # n % 4 != 0 -> dense
    "wrap": (4, [(64, 16)] * (GRID_CAP + 1) + [(1,)]),            # more matrices than the capped grid has workgroups
    # the dense part a multiple of 4 elements (as in a real model): every P on a 16-byte boundary, which takes
    # the orthonormalisation to its row-sweeping kernel for R in {4, 8, 16, 32}
    "r4a": (4, [(40, 16), (8,), (20, 24)]),
    "r8a": (8, [(257, 72), (4,), (72, 260), (60,)]),
    "r16a": (16, [(64, 64), (64,), (1000, 80)]),
    "r32a": (32, [(1000, 128), (128, 1000)]),                     # no dense span at all
}
DENSE_2D = {"r16": [(63, 64)], "r4": [(66, 70)]}


def make_plan(case):
    """(plan, span): the case's tensors at 64-aligned offsets, through the real rule of LowRankPlan."""
    rank, tensors = CASES[case]
    names, shapes, offsets, off = [], {}, {}, 0
    for i, shape in enumerate(tensors):
        off = (off + 63) // 64 * 64
        names.append(f"t{i}")
        shapes[f"t{i}"], offsets[f"t{i}"] = shape, off
        off += int(np.prod(shape))
    plan = LowRankPlan(names, shapes, offsets, rank)
    want = [s for s in tensors if len(s) == 2 and s not in DENSE_2D.get(case, [])]
    assert [(m, n) for _, m, n, _, _ in plan.mats] == want, "the compression rule chose other tensors"
    return plan, (off + 63) // 64 * 64 + 64


def covered(plan, span):
    mask = np.zeros(span, dtype=bool)
    for off, m, n, _, _ in plan.mats:
        mask[off:off + m * n] = True
    comp = mask.copy()
    for a, b in plan.dense:
        mask[a:b] = True
    return mask, comp


def make_inputs(plan, span, seed, scale=1e-2):
    """(sync, master, e) fp32 numpy: Gaussian, with a few exact zeros, both signed zeros and one row of 1e-30-scale
    values per matrix.  ``e`` is non-zero everywhere, also where the ops must leave it alone."""
    rng = np.random.default_rng(seed)
    master = rng.standard_normal(span).astype(np.float32)
    sync = (master + scale * rng.standard_normal(span)).astype(np.float32)
    e = (scale * 0.1 * rng.standard_normal(span)).astype(np.float32)
    for off, m, n, _, _ in plan.mats:
        z = off + rng.integers(0, m * n, 4)
        sync[z[0]] = master[z[0]] = e[z[0]] = 0.0                    # acc = +0
        sync[z[1]], master[z[1]], e[z[1]] = -0.0, 0.0, -0.0          # acc = -0
        sync[z[2]] = master[z[2]]                                    # acc = e
        e[z[3]] = 0.0
        r = off + (m // 2) * n
        for buf in (sync, master, e):
            buf[r:r + n] = (1e-30 * rng.standard_normal(n)).astype(np.float32)
    return sync, master, e


class State:
    """The buffers of one worker on ``dev``, each inside guards."""

    def __init__(self, plan, span, dev, sync, master, e, mom=None, shadow=False, q=None, q0=None, s_out=True):
        self.plan, self.span, self.dev = plan, span, dev
        w1, w2 = ops.lowrank_wire_elems(plan)
        self.q0_np = plan.init_q().numpy() if q0 is None else q0
        parts = dict(sync=sync, master=master, resid=e, mom=np.zeros(span, np.float32) if mom is None else mom,
                     q=self.q0_np if q is None else q, q0=self.q0_np, wire1=np.full(w1, 7.0, np.float32),
                     wire2=np.full(w2, 7.0, np.float32))
        if s_out:
            parts["s_out"] = np.full(span, 5.0, np.float32)
        self.full = {}
        for k, v in parts.items():
            self.full[k], t = guarded_f32(torch.from_numpy(np.ascontiguousarray(v)), dev)
            setattr(self, k, t)
        if not s_out:
            self.s_out = None
        self.shadow = self.master.to(torch.bfloat16) if shadow else None

    def np(self, name):
        return getattr(self, name).detach().float().cpu().numpy().copy()

    def guards_ok(self):
        return all(f32_guards_intact(f) for f in self.full.values())


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    an, bn = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(an, bn) and np.array_equal(a.view(np.int32)[~an], b.view(np.int32)[~bn]))


def ratio(got, exact, bound):
    err = np.abs(got.astype(np.float64) - exact)
    assert np.all(err[bound == 0] == 0), "a sum of zeros must be zero"
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def full_step(st, inv_w=1.0, first=True, presum=1.0):
    """One outer step of one worker through the four ops; ``presum`` scales both wire buffers where an all-reduce
    would have summed them.  Returns numpy copies of what went over the wire."""
    plan = st.plan
    ops.lowrank_project(st.sync, st.master, st.resid, st.q, st.wire1, plan)
    out = {"P": st.np("wire1"), "acc": st.np("resid")}
    st.wire1.mul_(presum)
    ops.lowrank_orthonormalize(st.wire1, plan)
    out["Ph"] = st.np("wire1")
    ops.lowrank_backproject(st.resid, st.wire1, st.wire2, plan)
    st.wire2.mul_(presum)
    out["Qsum"] = st.np("wire2")
    ops.outer_nesterov_lowrank(st.master, st.sync, st.resid, st.wire1, st.wire2, st.q, st.q0, st.mom, st.shadow, plan,
                               inv_w, LR, MU, first, st.s_out)
    return out


# ------------------------------------------------------------------------------------------ 1. dot products
def check_project(case, dev, seed=0):
    plan, span = make_plan(case)
    R = plan.rank
    sync, master, e = make_inputs(plan, span, seed)
    st = State(plan, span, dev, sync, master, e, s_out=False)
    ops.lowrank_project(st.sync, st.master, st.resid, st.q, st.wire1, plan)
    assert st.guards_ok(), "lowrank_project wrote outside a buffer"
    assert bits_equal(st.np("sync"), sync) and bits_equal(st.np("master"), master) and bits_equal(st.np("q"), st.q0_np)
    _, comp = covered(plan, span)
    acc = lo.acc32(sync, master, e)
    got_e, wire = st.np("resid"), st.np("wire1")
    assert bits_equal(got_e[comp], acc[comp]), "acc != (sync - master) + e, bitwise"
    assert bits_equal(got_e[~comp], e[~comp]), "the residual outside the compressed matrices was touched"
    # dense spans: nd_pseudograd's bits
    pg = torch.empty(span, device=dev)
    ops.pseudograd(st.sync, st.master, pg)
    pg = pg.cpu().numpy()
    for (a, b), pre in zip(plan.dense, plan.dense_pre):
        assert bits_equal(wire[pre:pre + b - a], pg[a:b]), "dense wire != nd_pseudograd"
    worst = 0.0
    for off, m, n, po, qo in plan.mats:
        exact, bound = lo.dot_bound(acc[off:off + m * n].reshape(m, n), st.q0_np[qo:qo + n * R].reshape(n, R), n)
        worst = max(worst, ratio(wire[po:po + m * R].reshape(m, R), exact, bound))
    assert worst <= 1.0, f"P: error / bound = {worst}"
    return worst


def _unit_columns(rng, m, R):
    P = rng.standard_normal((m, R))
    return (P / np.linalg.norm(P, axis=0)).astype(np.float32)


def check_backproject(case, dev, seed=1):
    plan, span = make_plan(case)
    R = plan.rank
    rng = np.random.default_rng(seed)
    _, _, acc = make_inputs(plan, span, seed, scale=1.0)
    wire1 = np.full(plan.wire1_elems, 3.0, np.float32)
    for _, m, _, po, _ in plan.mats:
        wire1[po:po + m * R] = _unit_columns(rng, m, R).reshape(-1)
    st = State(plan, span, dev, acc, acc, acc, s_out=False)
    st.wire1.copy_(torch.from_numpy(wire1))
    ops.lowrank_backproject(st.resid, st.wire1, st.wire2, plan)
    assert st.guards_ok() and bits_equal(st.np("resid"), acc) and bits_equal(st.np("wire1"), wire1)
    got, worst = st.np("wire2"), 0.0
    for off, m, n, po, qo in plan.mats:
        exact, bound = lo.dot_bound(acc[off:off + m * n].reshape(m, n).T, wire1[po:po + m * R].reshape(m, R), m)
        worst = max(worst, ratio(got[qo:qo + n * R].reshape(n, R), exact, bound))
    assert worst <= 1.0, f"Q_loc: error / bound = {worst}"
    return worst


# ------------------------------------------------------------------------------------------ 2. orthonormalisation
def check_orthonormalize(case, dev, seed=2):
    """Gaussian P (kappa <= 4, asserted): every element within 4 x the fp32 sequential twin's largest error against
    the float64 oracle, and max|P^T P - I| within 4 x the twin's."""
    plan, span = make_plan(case)
    R = plan.rank
    rng = np.random.default_rng(seed)
    wire1 = np.full(plan.wire1_elems, 3.0, np.float32)
    for _, m, _, po, _ in plan.mats:
        wire1[po:po + m * R] = rng.standard_normal(m * R).astype(np.float32)
    full, w = guarded_f32(torch.from_numpy(wire1), dev)
    ops.lowrank_orthonormalize(w, plan)
    assert f32_guards_intact(full)
    got = w.cpu().numpy()
    assert bits_equal(got[:plan.dense_total], wire1[:plan.dense_total]), "the dense part of wire 1 was touched"
    worst = worst_orth = 0.0
    eye = np.eye(R)
    for _, m, _, po, _ in plan.mats:
        P = wire1[po:po + m * R].reshape(m, R)
        kappa = lo.cond(P)
        assert kappa <= 4.0, f"badly conditioned draw: kappa = {kappa} for {m} x {R}"
        want = lo.mgs(P, np.float64)
        twin = lo.mgs(P, np.float32, sequential=True).astype(np.float64)
        G = got[po:po + m * R].reshape(m, R).astype(np.float64)
        assert np.isfinite(G).all()
        tw_err, tw_orth = np.abs(twin - want).max(), np.abs(twin.T @ twin - eye).max()
        err, orth = np.abs(G - want).max(), np.abs(G.T @ G - eye).max()
        worst, worst_orth = max(worst, err / (4 * tw_err)), max(worst_orth, orth / (4 * tw_orth))
    assert worst <= 1.0 and worst_orth <= 1.0, f"P^: error / (4 x twin) = {worst}, orthogonality / (4 x twin) = {worst_orth}"
    return worst, worst_orth


def check_orthonormalize_edges(dev):
    plan, _ = make_plan("r8")
    R = plan.rank
    rng = np.random.default_rng(3)
    (_, m0, _, p0, _), (_, m1, _, p1, _) = plan.mats
    wire1 = np.zeros(plan.wire1_elems, np.float32)  # matrix 0: all zero
    P = rng.standard_normal((m1, R)).astype(np.float32)
    P[:, 3] = P[:, 1]  # a duplicated column
    wire1[p1:p1 + m1 * R] = P.reshape(-1)
    w = torch.from_numpy(wire1).to(dev)
    ops.lowrank_orthonormalize(w, plan)
    got = w.cpu().numpy()
    assert not got[p0:p0 + m0 * R].any(), "an all-zero P must stay all zero"
    G = got[p1:p1 + m1 * R].reshape(m1, R).astype(np.float64)
    assert np.isfinite(G).all()
    twin = lo.mgs(np.delete(P, 3, axis=1), np.float32, sequential=True).astype(np.float64)
    noise = 4 * np.abs(twin.T @ twin - np.eye(R - 1)).max()
    assert not G[:, 3].any() or abs(G[:, 1] @ G[:, 3]) <= noise, "the second copy is neither zero nor orthogonal"
    keep = [c for c in range(R) if c != 3]
    assert np.abs(G[:, keep].T @ G[:, keep] - np.eye(R - 1)).max() <= noise


# ------------------------------------------------------------------------------------------ 3. apply
def check_apply(case, dev, w, first, shadow, seed=4):
    """Master, sync, momentum and the bf16 shadow equal ``ops.outer_nesterov`` fed ``s_out``, bitwise, on every covered
    element; nothing else moves; ``e = fl(acc - fl(s * inv_w))``; ``s`` within the dot bound; Q = Q_sum * inv_w with
    the dead column re-seeded."""
    plan, span = make_plan(case)
    R = plan.rank
    rng = np.random.default_rng(seed + w)
    inv_w = 1.0 / w
    sync, master, acc = make_inputs(plan, span, seed)
    mom = (0.01 * rng.standard_normal(span)).astype(np.float32)
    st = State(plan, span, dev, sync, master, acc, mom=mom, shadow=shadow,
               q=rng.standard_normal(plan.wire2_elems).astype(np.float32))
    wire1 = (w * 0.01 * rng.standard_normal(plan.wire1_elems)).astype(np.float32)  # dense part: a sum of W workers
    wire2 = (w * rng.standard_normal(plan.wire2_elems)).astype(np.float32)
    for i, (_, m, n, po, qo) in enumerate(plan.mats):
        wire1[po:po + m * R] = _unit_columns(rng, m, R).reshape(-1)
        if i % 2 == 0:
            wire2[qo:qo + n * R].reshape(n, R)[:, R - 1] = 0.0  # a dead direction
    st.wire1.copy_(torch.from_numpy(wire1))
    st.wire2.copy_(torch.from_numpy(wire2))
    old = {k: getattr(st, k).clone() for k in ("master", "sync", "mom")}
    old_sh = st.shadow.clone() if shadow else None
    ops.outer_nesterov_lowrank(st.master, st.sync, st.resid, st.wire1, st.wire2, st.q, st.q0, st.mom, st.shadow, plan,
                               inv_w, LR, MU, first, st.s_out)
    assert st.guards_ok() and bits_equal(st.np("wire1"), wire1) and bits_equal(st.np("wire2"), wire2)
    mask, comp = covered(plan, span)
    s = st.np("s_out")
    assert bits_equal(s[~mask], np.full(span, 5.0, np.float32)[~mask])
    delta = torch.from_numpy(np.where(mask, s, 0.0).astype(np.float32)).to(dev)
    ops.outer_nesterov(old["master"], old["sync"], delta, old["mom"], old_sh, inv_w, LR, MU, first)
    for name in ("master", "sync", "mom"):
        got, want = st.np(name), old[name].cpu().numpy()
        assert bits_equal(got[mask], want[mask]), f"{name} != nd_outer_nesterov's on a covered element"
    for name, before in (("master", master), ("sync", sync), ("mom", mom)):
        assert bits_equal(st.np(name)[~mask], before[~mask]), f"{name} changed outside the table"
    if shadow:
        got, want = st.shadow.float().cpu().numpy(), old_sh.float().cpu().numpy()
        assert bits_equal(got[mask], want[mask]), "bf16 shadow"
        assert bits_equal(got[~mask], torch.from_numpy(master).to(torch.bfloat16).float().numpy()[~mask])
    want_e = acc - s * np.float32(inv_w)  # two fp32 roundings
    got_e = st.np("resid")
    assert bits_equal(got_e[comp], want_e[comp]), "e != fl(acc - fl(s * inv_w))"
    assert bits_equal(got_e[~comp], acc[~comp])
    worst, q_new = 0.0, st.np("q")
    for (a, b), pre in zip(plan.dense, plan.dense_pre):
        assert bits_equal(s[a:b], wire1[pre:pre + b - a])
    for i, (off, m, n, po, qo) in enumerate(plan.mats):
        Ph, Qs = wire1[po:po + m * R].reshape(m, R), wire2[qo:qo + n * R].reshape(n, R)
        exact, bound = lo.dot_bound(Ph, Qs.T, R)
        worst = max(worst, ratio(s[off:off + m * n].reshape(m, n), exact, bound))
        want_q = Qs * np.float32(inv_w)
        if i % 2 == 0:
            want_q[:, R - 1] = st.q0_np[qo:qo + n * R].reshape(n, R)[:, R - 1]
        assert bits_equal(q_new[qo:qo + n * R].reshape(n, R), want_q), "Q != Q_sum * inv_w (dead column: Q0)"
    assert worst <= 1.0, f"s: error / bound = {worst}"
    return worst


def check_reseed_nonfinite(dev):
    plan, span = make_plan("r8")
    R = plan.rank
    z = np.zeros(span, np.float32)
    st = State(plan, span, dev, z, z, z, s_out=False)
    st.wire1.zero_()
    st.wire2.fill_(1.0)
    (_, _, n0, _, q0), (_, _, n1, _, q1) = plan.mats
    st.wire2[q0 + 2] = float("nan")   # column 2 of matrix 0
    st.wire2[q1 + R + 5] = float("inf")  # column 5 of matrix 1
    ops.outer_nesterov_lowrank(st.master, st.sync, st.resid, st.wire1, st.wire2, st.q, st.q0, st.mom, None, plan,
                               0.5, LR, MU, True, None)
    q = st.np("q")
    assert np.isfinite(q).all()
    for qo, n, c in ((q0, n0, 2), (q1, n1, 5)):
        got, want = q[qo:qo + n * R].reshape(n, R), np.full((n, R), 0.5, np.float32)
        want[:, c] = st.q0_np[qo:qo + n * R].reshape(n, R)[:, c]
        assert bits_equal(got, want)


# ------------------------------------------------------------------------------------------ 4. exact recovery
def _integer_lowrank(plan, span, rp, seed):
    """sync with acc = A B^T per compressed matrix (small integers: exact in fp32), master = e = 0."""
    rng = np.random.default_rng(seed)
    sync = np.zeros(span, np.float32)
    for off, m, n, _, _ in plan.mats:
        A, B = rng.integers(-2, 3, (m, rp)), rng.integers(-2, 3, (n, rp))
        sync[off:off + m * n] = (A @ B.T).astype(np.float32).reshape(-1)
    return sync


def check_exact_recovery(case, dev, seed=5):
    """acc = A B^T of rank R' <= R at W = 1: one step leaves |e| and |d - acc| within the composed bound, R' = R + 1
    leaves a clearly non-zero residual.

    Composition (first order, per matrix, u = 2^-24).  With G = |P^| (|P^|^T |acc|) >= |s| element by element, the
    three products contribute their check-1 errors: (n + 2) u on P, (m + 2) u on Q_loc, (R + 2) u on s.  The error of
    P (and Gram-Schmidt's own R dot products of length m per column, (m + 2) R u) reaches the result through the
    orthonormal basis, whose sensitivity to a perturbation of P is kappa(P) (sigma_1 / sigma_R' of the exact P).
    So |e|, |d - acc| <= u * kappa * [(n + 2) + (m + 2)(R + 1) + (R + 2)] * max(G)."""
    plan, span = make_plan(case)
    R = plan.rank
    z = np.zeros(span, np.float32)
    worst = 0.0
    for rp in sorted({1, R}):
        sync = _integer_lowrank(plan, span, rp, seed + rp)
        st = State(plan, span, dev, sync, z, z)
        out = full_step(st)
        e, s = st.np("resid"), st.np("s_out")
        for off, m, n, po, qo in plan.mats:
            acc = sync[off:off + m * n].reshape(m, n).astype(np.float64)
            sv = np.linalg.svd(acc @ st.q0_np[qo:qo + n * R].reshape(n, R).astype(np.float64), compute_uv=False)
            rank = int((sv > sv[0] * 1e-9).sum())
            kappa = sv[0] / sv[rank - 1]
            Ph = np.abs(out["Ph"][po:po + m * R].reshape(m, R).astype(np.float64))
            G = Ph @ (Ph.T @ np.abs(acc))
            tol = lo.U * kappa * ((n + 2) + (m + 2) * (R + 1) + (R + 2)) * G.max()
            err = max(np.abs(e[off:off + m * n]).max(), np.abs(s[off:off + m * n].reshape(m, n) - acc).max())
            assert err <= tol, f"rank {rp} in {R}: |e| = {err} > {tol} for {m} x {n}"
            worst = max(worst, err / tol)
    sync = _integer_lowrank(plan, span, R + 1, seed)
    st = State(plan, span, dev, sync, z, z)
    full_step(st)
    e = st.np("resid")
    for off, m, n, _, _ in plan.mats:
        if min(m, n) > R + 1:
            assert np.linalg.norm(e[off:off + m * n]) > 1e-3 * np.linalg.norm(sync[off:off + m * n]), \
                "rank R + 1 went through R columns"
    return worst


# ------------------------------------------------------------------------------------------ 5. conservation
def check_conservation(case, dev, steps=6, seed=6):
    """Constant g, W = 1: sum_t d_t + e_T = T g within (2T + 2) u max|.| per element (two roundings per step: acc and
    e), and ||e_t||_F <= 1.001 ||g||_F per matrix.  g is rank-R integers plus 1e-3 noise: for a pseudo-gradient whose
    energy is NOT mostly inside rank R the residual of any rank-R projection legitimately keeps growing (about t ||g||
    for a Gaussian g), so the norm property is one of near-low-rank inputs only."""
    plan, span = make_plan(case)
    R = plan.rank
    rng = np.random.default_rng(seed)
    g = _integer_lowrank(plan, span, R, seed)
    _, comp = covered(plan, span)
    g = (g + comp * 1e-3 * rng.standard_normal(span)).astype(np.float32)
    for a, b in plan.dense:
        g[a:b] = rng.standard_normal(b - a).astype(np.float32)
    z = np.zeros(span, np.float32)
    st = State(plan, span, dev, z, -g, z)  # sync = 0: sync - master = g exactly
    total, big = np.zeros(span), float(np.abs(g).max())
    for t in range(steps):
        st.sync.zero_()
        st.master.copy_(torch.from_numpy(-g))
        out = full_step(st, first=(t == 0))
        d = st.np("s_out").astype(np.float64)  # W = 1: d = s
        total += d
        e = st.np("resid")
        big = max(big, float(np.abs(out["acc"][comp]).max()), float(np.abs(d[comp]).max()))
        for off, m, n, _, _ in plan.mats:
            ne, ng = np.linalg.norm(e[off:off + m * n].astype(np.float64)), np.linalg.norm(g[off:off + m * n].astype(np.float64))
            assert ne <= 1.001 * ng, f"step {t}: ||e|| = {ne} > ||g|| = {ng}"
    mask, _ = covered(plan, span)
    err = np.abs(total + np.where(comp, e, 0.0) - steps * g.astype(np.float64))[mask].max()
    tol = (2 * steps + 2) * lo.U * big
    assert err <= tol, f"sum d + e - T g = {err} > {tol}"
    return err / tol


# ------------------------------------------------------------------------------------------ 6 / 7
def check_zero_step(case, dev, seed=7):
    plan, span = make_plan(case)
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal(span).astype(np.float32)
    st = State(plan, span, dev, theta, theta, np.zeros(span, np.float32), shadow=True,
               q=rng.standard_normal(plan.wire2_elems).astype(np.float32))
    full_step(st, first=True)
    mask, comp = covered(plan, span)
    for name in ("master", "sync", "mom", "resid", "q", "s_out", "wire1", "wire2"):
        assert np.isfinite(st.np(name)).all(), name
    assert not st.np("s_out")[mask].any() and not st.np("resid")[comp].any() and not st.np("mom")[mask].any()
    assert bits_equal(st.np("master"), theta) and bits_equal(st.np("sync"), theta)
    assert bits_equal(st.np("q"), st.q0_np), "every direction was dead: Q is Q0 again"


def check_repeatable(case, dev, seed=8):
    plan, span = make_plan(case)
    sync, master, e = make_inputs(plan, span, seed)
    runs = []
    for _ in range(2):
        st = State(plan, span, dev, sync, master, e)
        out = full_step(st, inv_w=0.5, first=False, presum=2.0)
        out.update({k: st.np(k) for k in ("resid", "q", "master", "sync", "mom")})
        runs.append(out)
    for k in runs[0]:
        assert bits_equal(runs[0][k], runs[1][k]), f"{k} differs between two runs of the same inputs"


# ------------------------------------------------------------------------------------------ 10. one worker
TINY = dict(vocab_size=256, hidden_size=128, intermediate_size=320, num_attention_heads=4, num_key_value_heads=2,
            num_hidden_layers=2, max_position_embeddings=64)


def check_diloco_one_worker(dev, dtype, rank=8, steps=2):
    """``Diloco(lowrank=8)`` on the tiny GQA Llama next to a dense twin, two outer steps of the same drift."""
    from nanodiloco_amd.config import LlamaConfig
    from nanodiloco_amd.models import LlamaForCausalLM
    from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
    from nanodiloco_amd.parallel.diloco import Diloco
    from nanodiloco_amd.parallel.dist import DistEnv
    from nanodiloco_amd.parallel.transports import DenseTransport, LowRankTransport
    made = []
    for r in (rank, 0):
        m = LlamaForCausalLM(LlamaConfig(**TINY), dev, dtype).init_weights(7)
        dl = Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store, lr=LR, momentum=MU), 1, 100, 2,
                    env=DistEnv(device=dev), comm_dtype=torch.float32, lowrank=r)
        made.append((m, dl))
    (m, dl), (m2, dl2) = made
    assert isinstance(dl.transport, LowRankTransport) and isinstance(dl2.transport, DenseTransport)
    plan, st = dl.transport.plan, m.store
    assert len(plan) == 2 + 7 * TINY["num_hidden_layers"]  # embedding, lm head, q / k / v / o / gate / up / down
    assert dl.transport.bytes_per_step == 4 * sum(ops.lowrank_wire_elems(plan)) < 4 * st.numel // 4
    mask, comp = covered(plan, st.numel)
    for s in range(steps):
        drift = (0.01 / (s + 1)) * torch.randn(st.numel, generator=torch.Generator().manual_seed(s)).to(dev)
        drift *= torch.from_numpy(mask).to(dev)  # the padding between tensors never moves
        for mm, dd in ((m, dl), (m2, dl2)):
            mm.store.master.add_(drift)
            dd.outer_step()
        assert torch.equal(st.master, dl.sync) and torch.equal(st.shadow, st.master.to(st.shadow.dtype))
        assert bool(torch.isfinite(st.master).all())
        for name in st.names:
            if "norm" in name:
                assert torch.equal(st.master_view(name), m2.store.master_view(name)), name
        e = dl.lowrank_residual.cpu().numpy()
        assert e[comp].any() and not e[~comp].any()
    assert not torch.equal(st.master, m2.store.master)  # rank 8 did not carry everything
    assert dl.outer_step_count == steps and dl.outer_optimizer.step_count == steps
