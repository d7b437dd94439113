"""Low-rank (PowerSGD: Vogels, Karimireddy, Jaggi 2019) transport of the DiLoCo pseudo-gradient with error feedback
(``csrc/lowrank_comm.hip``; format and rules in docs/DESIGN.md "Low-rank transport").

Every compressed matrix [m, n] of the flat vector travels as two thin factors P [m, R] and Q [n, R].  Both are
linear in the pseudo-gradient, so both are all-reduced: bytes sent and received do not depend on the number of workers.

  ``nd_lowrank_project``          acc = (theta_sync - theta_local) + e -> e;  P = acc Q -> wire 1; dense spans: sync - local
  -- all-reduce(SUM) of wire 1 = [dense | all P] --
  ``nd_lowrank_orthonormalize``   modified Gram-Schmidt over the R columns of every summed P, in column order
  ``nd_lowrank_backproject``      Q_loc = acc^T P^ -> wire 2 (acc read from e)
  -- all-reduce(SUM) of wire 2 = [all Q] --
  ``nd_outer_nesterov_lowrank``   s = sum_c P^[i,c] Q_sum[j,c];  d = s / W;  e = acc - d;  ``nd_outer_nesterov``'s update
                                  with d;  Q <- Q_sum / W, a dead column re-seeded from Q0

Orthonormalisation drops (zeroes) a column whose norm is zero or not finite, and one that lost 12 bits of its norm to
the columns before it (numerically dependent); its Q column then comes back all zero and is re-seeded.

Every function has a PyTorch implementation with the same formulas in fp32 (CPU path, ``--ops torch``).  The dot
products associate differently there, so -- unlike the top-k transport -- HIP and PyTorch results agree to rounding, not
bit for bit; each path on its own is deterministic.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _ext
from .optim import outer_nesterov

MAX_RANK = 32
Q_SEED = 0x51F15EED  # Q0 of matrix i is drawn from a CPU generator seeded with Q_SEED + i
DEPENDENT = 2.0 ** -24  # on squared norms: a column that kept less than 2^-12 of its norm is dropped


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n


class LowRankPlan:
    """Which tensors of a flat parameter vector travel as factors (``mats``: rows ``(offset, m, n, p_off, q_off)``)
    and which as plain fp32 (``dense``: ``(start, end)`` spans, neighbours merged).  A 2-D tensor [m, n] is compressed
    when ``min(m, n) >= 4 * rank``, ``n % 4 == 0`` and its offset is a multiple of 4; every tensor is taken on its own.
    Wire 1 is ``[dense | all P]`` (``p_off`` counts from its start), wire 2 and the Q state are ``[all Q]``.
    Built once from ``names`` / ``shapes`` / ``offsets`` (a ``ParamStore``'s); no tensor is allocated until a table
    is asked for."""

    def __init__(self, names: Sequence[str], shapes: Dict[str, Tuple[int, ...]], offsets: Dict[str, int], rank: int):
        mats, dense, self.mat_names = [], [], []
        for name in names:
            shape, off = tuple(int(s) for s in shapes[name]), int(offsets[name])
            if len(shape) == 2 and self.compressible(shape[0], shape[1], rank) and off % 4 == 0:
                mats.append((off, shape[0], shape[1]))
                self.mat_names.append(name)
            elif _numel(shape):
                dense.append((off, off + _numel(shape)))
        self._build(mats, dense, rank)

    @staticmethod
    def compressible(m: int, n: int, rank: int) -> bool:
        return min(m, n) >= 4 * rank and n % 4 == 0

    @classmethod
    def from_layout(cls, mats: Sequence[Tuple[int, int, int]], dense: Sequence[Tuple[int, int]], rank: int) -> "LowRankPlan":
        """A plan over hand-made ``(offset, m, n)`` matrices and ``(start, end)`` dense spans (tests and tools);
        nothing is checked here -- the launchers (HIP) and :meth:`check` (PyTorch) do that."""
        self = cls.__new__(cls)
        self.mat_names = [f"m{i}" for i in range(len(mats))]
        self._build([tuple(int(x) for x in r) for r in mats], [tuple(int(x) for x in r) for r in dense], rank)
        return self

    def _build(self, mats, dense, rank):
        if not 1 <= int(rank) <= MAX_RANK:
            raise ValueError(f"low-rank transport keeps 1 <= rank <= {MAX_RANK} columns, not {rank}")
        self.rank = R = int(rank)
        self.dense: List[Tuple[int, int]] = []
        for a, b in sorted(dense):
            if self.dense and self.dense[-1][1] == a:
                self.dense[-1] = (self.dense[-1][0], b)
            else:
                self.dense.append((a, b))
        self.dense_pre = [0]
        for a, b in self.dense:
            self.dense_pre.append(self.dense_pre[-1] + (b - a))
        self.dense_total = self.dense_pre[-1]
        p, q = self.dense_total, 0
        self.mats: List[Tuple[int, int, int, int, int]] = []
        for off, m, n in mats:
            self.mats.append((off, m, n, p, q))
            p += m * R
            q += n * R
        self.wire1_elems, self.wire2_elems = p, q
        self.end = max([0] + [off + m * n for off, m, n, _, _ in self.mats] + [b for _, b in self.dense])
        self._host = self._host_dense = None
        self._dev: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor]] = {}

    @classmethod
    def from_store(cls, store, rank: int) -> "LowRankPlan":
        return cls(store.names, store.shapes, store.offsets, rank)

    def __len__(self):
        return len(self.mats)

    @property
    def compressed_elems(self) -> int:
        return sum(m * n for _, m, n, _, _ in self.mats)

    def host_tables(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(matrix table ``[nmat * 5]``, dense table ``[2 S + S + 1]``) as int64 CPU tensors."""
        if self._host is None:
            self._host = torch.tensor([x for row in self.mats for x in row], dtype=torch.int64)
            self._host_dense = torch.tensor([x for ab in self.dense for x in ab] + self.dense_pre, dtype=torch.int64)
        return self._host, self._host_dense

    def device_tables(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            h, hd = self.host_tables()
            t = self._dev[device] = (h.to(device), hd.to(device))
        return t

    def init_q(self, seed: int = Q_SEED) -> torch.Tensor:
        """Q0 (fp32, CPU, ``wire2_elems``): standard normal, matrix i from a CPU generator seeded ``seed + i`` -- the
        same on every worker and in every resumed run, without communication."""
        out = torch.empty(self.wire2_elems, dtype=torch.float32)
        for i, (_, _, n, _, qo) in enumerate(self.mats):
            g = torch.Generator().manual_seed(int(seed) + i)
            out[qo:qo + n * self.rank] = torch.randn(n * self.rank, generator=g, dtype=torch.float32)
        return out

    def check(self, what: str, span: int, w1: int, w2: int) -> None:
        """The launchers' table checks, for the PyTorch path."""
        R = self.rank
        for off, m, n, po, qo in self.mats:
            if off < 0 or m < 1 or n < 1 or off % 4 or n % 4 or qo % 4 or off + m * n > span:
                raise ValueError(f"{what}: matrix row ({off}, {m}, {n}) is outside [0, {span}) or misaligned")
            if po < 0 or po + m * R > w1 or qo < 0 or qo + n * R > w2:
                raise ValueError(f"{what}: factor offsets ({po}, {qo}) are outside their buffers")
        for a, b in self.dense:
            if a < 0 or b <= a or b > span:
                raise ValueError(f"{what}: dense span [{a}, {b}) is outside [0, {span})")
        if self.dense_total > w1:
            raise ValueError(f"{what}: the dense spans do not fit wire buffer 1")


def lowrank_wire_elems(plan: LowRankPlan) -> Tuple[int, int]:
    """fp32 elements of the two wire buffers: ``(dense + sum m R, sum n R)``."""
    return plan.wire1_elems, plan.wire2_elems


def _f32(what: str, **tensors) -> None:
    for name, t in tensors.items():
        if t is not None and (t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous()):
            raise ValueError(f"{what}: {name} must be a contiguous 1-D fp32 tensor")


def _sizes(what: str, plan: LowRankPlan, span: int, wire1=None, wire2=None, q=None, q0=None, **flat) -> None:
    for name, t in flat.items():
        if t is not None and t.numel() != span:
            raise ValueError(f"{what}: {name} has {t.numel()} elements, the span has {span}")
    if wire1 is not None and wire1.numel() != plan.wire1_elems:
        raise ValueError(f"{what}: wire buffer 1 has {wire1.numel()} elements, the plan needs {plan.wire1_elems}")
    for name, t in (("wire buffer 2", wire2), ("q", q), ("q0", q0)):
        if t is not None and t.numel() != plan.wire2_elems:
            raise ValueError(f"{what}: {name} has {t.numel()} elements, the plan needs {plan.wire2_elems}")


def _tables(plan: LowRankPlan, device):
    h, hd = plan.host_tables()
    d, dd = plan.device_tables(device)
    return _ext.ptr(h), _ext.ptr(d), len(plan.mats), _ext.ptr(hd), _ext.ptr(dd), len(plan.dense)


def lowrank_project(sync: torch.Tensor, master: torch.Tensor, resid: torch.Tensor, q: torch.Tensor,
                    wire1: torch.Tensor, plan: LowRankPlan) -> None:
    """Compressed matrices: ``acc = (sync - master) + resid`` (two fp32 operations in this order) is written back
    into ``resid`` and ``P = acc Q`` into ``wire1``; dense spans: ``sync - master`` into the dense part of ``wire1``
    (``resid`` is not touched there)."""
    what, span = "lowrank_project", master.numel()
    _f32(what, sync=sync, master=master, resid=resid, q=q, wire1=wire1)
    _sizes(what, plan, span, wire1=wire1, q=q, sync=sync, resid=resid)
    R = plan.rank
    if _ext.use_hip(master):
        ht, dt, nm, hd, dd, S = _tables(plan, master.device)
        _ext.check(_ext.lib().nd_lowrank_project(_ext.ptr(sync), _ext.ptr(master), _ext.ptr(resid), _ext.ptr(q),
                                                 _ext.ptr(wire1), ht, dt, nm, hd, dd, S, R, span, wire1.numel(),
                                                 q.numel(), _ext.stream_ptr(master.device)), "nd_lowrank_project")
        return
    plan.check(what, span, wire1.numel(), q.numel())
    for off, m, n, po, qo in plan.mats:
        acc = torch.sub(sync[off:off + m * n], master[off:off + m * n]).add_(resid[off:off + m * n])
        resid[off:off + m * n] = acc
        torch.mm(acc.view(m, n), q[qo:qo + n * R].view(n, R), out=wire1[po:po + m * R].view(m, R))
    for (a, b), pre in zip(plan.dense, plan.dense_pre):
        torch.sub(sync[a:b], master[a:b], out=wire1[pre:pre + b - a])


def lowrank_orthonormalize(wire1: torch.Tensor, plan: LowRankPlan) -> None:
    """Modified Gram-Schmidt over the R columns of every P in ``wire1``, in column order, in place.  A column whose
    norm is zero, not finite or below 2^-12 of what it was before the earlier columns were taken out becomes all
    zero; nothing non-finite is ever written."""
    what = "lowrank_orthonormalize"
    _f32(what, wire1=wire1)
    _sizes(what, plan, 0, wire1=wire1)
    R = plan.rank
    if _ext.use_hip(wire1):
        ht, dt, nm, _, _, _ = _tables(plan, wire1.device)
        _ext.check(_ext.lib().nd_lowrank_orthonormalize(_ext.ptr(wire1), ht, dt, nm, R, wire1.numel(),
                                                        _ext.stream_ptr(wire1.device)), "nd_lowrank_orthonormalize")
        return
    for _, m, _, po, _ in plan.mats:
        if po < 0 or po + m * R > wire1.numel():
            raise ValueError(f"{what}: factor offset {po} is outside wire buffer 1")
        P = wire1[po:po + m * R].view(m, R)
        for c in range(R):
            v = P[:, c]
            s0 = float((v * v).sum())
            for k in range(c):
                v.sub_(P[:, k] * (P[:, k] * v).sum())
            s1 = (v * v).sum()
            f1 = float(s1)
            if f1 > 0.0 and f1 < float("inf") and f1 > s0 * DEPENDENT:
                v.div_(s1.sqrt())
            else:
                v.zero_()


def lowrank_backproject(resid: torch.Tensor, wire1: torch.Tensor, wire2: torch.Tensor, plan: LowRankPlan) -> None:
    """``Q_loc = acc^T P^`` per compressed matrix into ``wire2``; ``acc`` is read from ``resid`` (where
    :func:`lowrank_project` left it), ``P^`` from ``wire1``."""
    what, span = "lowrank_backproject", resid.numel()
    _f32(what, resid=resid, wire1=wire1, wire2=wire2)
    _sizes(what, plan, span, wire1=wire1, wire2=wire2)
    R = plan.rank
    if _ext.use_hip(resid):
        ht, dt, nm, _, _, _ = _tables(plan, resid.device)
        _ext.check(_ext.lib().nd_lowrank_backproject(_ext.ptr(resid), _ext.ptr(wire1), _ext.ptr(wire2), ht, dt, nm, R,
                                                     span, wire1.numel(), wire2.numel(),
                                                     _ext.stream_ptr(resid.device)), "nd_lowrank_backproject")
        return
    plan.check(what, span, wire1.numel(), wire2.numel())
    for off, m, n, po, qo in plan.mats:
        torch.mm(resid[off:off + m * n].view(m, n).t(), wire1[po:po + m * R].view(m, R),
                 out=wire2[qo:qo + n * R].view(n, R))


def outer_nesterov_lowrank(master: torch.Tensor, sync: torch.Tensor, resid: torch.Tensor, wire1: torch.Tensor,
                           wire2: torch.Tensor, q: torch.Tensor, q0: torch.Tensor, mom: torch.Tensor,
                           shadow: Optional[torch.Tensor], plan: LowRankPlan, inv_w: float, lr: float, mu: float,
                           first: bool, s_out: Optional[torch.Tensor] = None) -> None:
    """The outer Nesterov update (``ops.outer_nesterov`` without drift) of every element the plan covers.  Compressed
    element (i, j): ``s = sum_c P^[i,c] Q_sum[j,c]``, ``d = s * inv_w``, ``resid = acc - d`` (the error feedback is
    taken against the AGGREGATED reconstruction); dense element: ``d = wire * inv_w``.  Then ``q <- Q_sum * inv_w``,
    any column that is all zero or not finite taken from ``q0``.  ``s_out`` (fp32, the span's length; tests and
    tools) receives ``s`` or the dense wire sum per covered element.  Elements no table row covers are not touched."""
    what, span = "outer_nesterov_lowrank", master.numel()
    _f32(what, master=master, sync=sync, resid=resid, wire1=wire1, wire2=wire2, q=q, q0=q0, mom=mom, s_out=s_out)
    _sizes(what, plan, span, wire1=wire1, wire2=wire2, q=q, q0=q0, sync=sync, resid=resid, mom=mom, s_out=s_out,
           shadow=shadow)
    R = plan.rank
    sh = shadow if (shadow is not None and shadow.data_ptr() != master.data_ptr()) else None
    if _ext.use_hip(master):
        ht, dt, nm, hd, dd, S = _tables(plan, master.device)
        _ext.check(_ext.lib().nd_outer_nesterov_lowrank(
            _ext.ptr(master), _ext.ptr(sync), _ext.ptr(resid), _ext.ptr(wire1), _ext.ptr(wire2), _ext.ptr(q),
            _ext.ptr(q0), _ext.ptr(mom), _ext.ptr(sh), _ext.dtcode(sh) if sh is not None else 0, _ext.ptr(s_out),
            ht, dt, nm, hd, dd, S, R, span, wire1.numel(), wire2.numel(), float(inv_w), float(lr), float(mu),
            1 if first else 0, _ext.stream_ptr(master.device)), "nd_outer_nesterov_lowrank")
        return
    plan.check(what, span, wire1.numel(), wire2.numel())

    def update(a, b, delta):
        outer_nesterov(master[a:b], sync[a:b], delta, mom[a:b], sh[a:b] if sh is not None else None, inv_w, lr, mu,
                       first)
        if s_out is not None:
            s_out[a:b] = delta

    for off, m, n, po, qo in plan.mats:
        qs = wire2[qo:qo + n * R].view(n, R)
        s = torch.mm(wire1[po:po + m * R].view(m, R), qs.t()).view(-1)
        e = resid[off:off + m * n]
        torch.sub(e, s * inv_w, out=e)
        update(off, off + m * n, s)
        qn = qs * inv_w
        dead = (~torch.isfinite(qn)).any(dim=0) | (qn == 0).all(dim=0)
        q[qo:qo + n * R].view(n, R).copy_(torch.where(dead[None, :], q0[qo:qo + n * R].view(n, R), qn))
    for (a, b), pre in zip(plan.dense, plan.dense_pre):
        update(a, b, wire1[pre:pre + b - a])
