"""In-test oracle of the top-k sparse transport (docs/DESIGN.md "Top-k sparse transport"), independent of
``nanodiloco_amd/ops/sparse_comm.py``: numpy fp32 for the two additions and the residual, integer logic for the
keys, the selection and the bf16 rounding.  Selection is literally
``sorted(range(m), key=lambda i: (-key[i], i))[:k]`` per chunk."""
import numpy as np

CHUNK = 4096
NONE = 0xFFFF


def pad16(b):
    return (b + 15) // 16 * 16


def nchunks(n):
    return -(-n // CHUNK)


def slot_bytes(n, k, bf16):
    return pad16(nchunks(n) * k * 2) + pad16(nchunks(n) * k * (2 if bf16 else 4))


def bf16_bits(x):
    """fp32 array -> uint16 bf16 bit patterns, round to nearest even in integer arithmetic (a NaN stays a NaN)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r[nan] = (u[nan] >> 16) | 0x40
    return r.astype(np.uint16)


def bf16_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def keys(acc):
    return acc.view(np.int32) & 0x7FFFFFFF


def select(sync, master, e, k, bf16):
    """Steps 1-4 for one worker.  Returns (idx uint16 [nch, k], val [nch, k] (fp32, or uint16 bf16 bits),
    the new residual, acc)."""
    sync, master, e = (np.ascontiguousarray(t, dtype=np.float32) for t in (sync, master, e))
    n = sync.size
    with np.errstate(all="ignore"):
        acc = (sync - master) + e  # two fp32 operations
    key = keys(acc).tolist()
    nch = nchunks(n)
    idx = np.full((nch, k), NONE, dtype=np.uint16)
    val = np.zeros((nch, k), dtype=np.uint16 if bf16 else np.float32)
    new_e = acc.copy()
    for c in range(nch):
        lo = c * CHUNK
        kc = key[lo:lo + CHUNK]
        sel = sorted(sorted(range(len(kc)), key=lambda i: (-kc[i], i))[:k])
        g = np.asarray(sel, dtype=np.int64) + lo
        idx[c, :len(sel)] = sel
        if bf16:
            bits = bf16_bits(acc[g])
            val[c, :len(sel)] = bits
            sent = bf16_to_f32(bits)
        else:
            val[c, :len(sel)] = acc[g]
            sent = acc[g]
        with np.errstate(all="ignore"):
            new_e[g] = acc[g] - sent
    return idx, val, new_e, acc


def pack(idx, val, fill=0):
    """The wire slot as uint8; the padding bytes (never written by the sender) hold ``fill``."""
    ib, vb = idx.tobytes(), val.tobytes()
    out = np.full(pad16(len(ib)) + pad16(len(vb)), fill, dtype=np.uint8)
    out[:len(ib)] = np.frombuffer(ib, dtype=np.uint8)
    off = pad16(len(ib))
    out[off:off + len(vb)] = np.frombuffer(vb, dtype=np.uint8)
    return out


def values_f32(val):
    return bf16_to_f32(val) if val.dtype == np.uint16 else val


def dense_sum(slots, n):
    """Step 6 up to the update: a zero fp32 span, plus worker 0's entries, plus worker 1's, ...; ``slots``:
    ``[(idx, val), ...]`` in worker order.  Indices of 0xFFFF are skipped."""
    out = np.zeros(n, dtype=np.float32)
    for idx, val in slots:
        v = values_f32(val)
        for c in range(idx.shape[0]):
            keep = idx[c] != NONE
            g = idx[c][keep].astype(np.int64) + c * CHUNK
            with np.errstate(all="ignore"):
                out[g] = out[g] + v[c][keep]
    return out
