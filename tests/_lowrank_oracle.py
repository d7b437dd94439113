"""Float64 oracle of the low-rank transport (ops/lowrank_comm.py), written from the formulas of docs/DESIGN.md
"Low-rank transport" with numpy only, plus the fp32 sequential Gram-Schmidt twin that sizes the orthonormalisation bound.

The dot products are compared through the standard forward bound of a length-L fp32 sum in any order, with or without
fma: ``|got - exact| <= (L + 2) * 2^-24 * sum_k |a_k| |b_k|`` (Higham, Accuracy and Stability, 3.5: gamma_L, with two
spare roundings for the store and a final product)."""
import numpy as np

U = 2.0 ** -24
DEPENDENT = 2.0 ** -24  # on squared norms, as ops/lowrank_comm.py


def acc32(sync, master, e):
    """``(sync - master) + e``: two fp32 operations in this order (bitwise reference)."""
    return (sync.astype(np.float32) - master.astype(np.float32)) + e.astype(np.float32)


def dot_bound(a, b, length):
    """(exact product, bound) of ``a @ b`` for fp32 inputs, both float64."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return a64 @ b64, (length + 2) * U * (np.abs(a64) @ np.abs(b64))


def mgs(P, dtype=np.float64, sequential=False):
    """Modified Gram-Schmidt over the columns of P in column order, in ``dtype``.  ``sequential``: every sum runs
    element by element in ``dtype`` (numpy's cumsum does not pair), the plain loop an fp32 implementation would be.
    A column with a zero or non-finite norm, or one below 2^-12 of its norm before the projections, becomes zero."""
    A = np.array(P, dtype=dtype, copy=True)

    def dot(x, y):
        prod = (x * y).astype(dtype)
        return np.cumsum(prod, dtype=dtype)[-1] if sequential else prod.sum(dtype=dtype)

    for c in range(A.shape[1]):
        s0 = dot(A[:, c], A[:, c])
        for k in range(c):
            A[:, c] = (A[:, c] - dot(A[:, k], A[:, c]) * A[:, k]).astype(dtype)
        s1 = dot(A[:, c], A[:, c])
        if s1 > 0 and np.isfinite(s1) and s1 > s0 * dtype(DEPENDENT):
            A[:, c] = (A[:, c] / np.sqrt(s1)).astype(dtype)
        else:
            A[:, c] = 0
    return A


def cond(P):
    s = np.linalg.svd(P.astype(np.float64), compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else float("inf")
