"""In-test oracle of the block-quantised transport (docs/DESIGN.md "Quantised outer transport"), shared by
tests/test_qcomm_*.py.  Written against the format alone: it uses none of ``nanodiloco_amd.ops.qcomm``."""
import torch

QB = 256


def qmax(bits):
    return {8: 127.0, 4: 7.0}[bits]


def quant(x, bits):
    """The ten-line block quantiser: x fp32 [nb, 256] -> (codes int8 [nb, 256], scales fp32 [nb])."""
    q = qmax(bits)
    amax = x.abs().amax(dim=1)                      # NaN propagates, inf stays inf
    scale = amax / q
    # an IEEE division: tensor / tensor (torch evaluates `scalar / tensor` as reciprocal * scalar, two roundings)
    inv = torch.where(amax > 0, torch.full_like(amax, q) / amax, torch.zeros_like(amax))
    codes = (x * inv[:, None]).round().clamp(-q, q)  # round: half to even
    bad = ~torch.isfinite(amax)
    scale[bad] = float("nan")
    codes[bad] = 0
    return codes.to(torch.int8), scale


def chunk(n, w):
    per = -(-n // w)
    return -(-per // QB) * QB


def chunk_bytes(c, bits):
    return c * bits // 8 + c // QB * 4


def pack(codes, scales, bits):
    """codes int8 [w, c], scales fp32 [w, c/256] -> the wire bytes, chunk after chunk: [codes][scales]."""
    out = []
    for cw, sw in zip(codes, scales):
        u = cw.to(torch.int16) & 0xFF
        if bits == 4:
            u = (u[0::2] & 0xF) | ((u[1::2] & 0xF) << 4)  # element 2i in the low nibble of byte i
        out += [u.to(torch.uint8), sw.contiguous().view(torch.uint8)]
    return torch.cat(out)


def unpack(buf, w, c, bits):
    """the wire bytes -> (codes int8 [w, c], scales fp32 [w, c/256])"""
    pb, cb = chunk_bytes(c, bits), c * bits // 8
    b = buf.cpu().view(w, pb)
    raw = b[:, :cb].to(torch.int16)
    if bits == 4:
        raw = torch.stack([raw & 0xF, raw >> 4], dim=-1).reshape(w, c)
        codes = torch.where(raw > 7, raw - 16, raw)
    else:
        codes = torch.where(raw > 127, raw - 256, raw)
    return codes.to(torch.int8), b[:, cb:].contiguous().view(torch.float32)


def quant_span(d, w, bits):
    """fp32 span d (length n) -> (codes [w, c], scales [w, c/256]) of its w chunks, zero-padded."""
    c = chunk(d.numel(), w)
    x = torch.zeros(w * c)
    x[: d.numel()] = d
    codes, scale = quant(x.view(-1, QB), bits)
    return codes.view(w, c), scale.view(w, c // QB)


def dequant(codes, scales):
    """code * scale per element, fp32, same shape as codes"""
    return codes.float() * scales.repeat_interleave(QB, dim=-1)


def reduce_chunks(codes, scales, bits):
    """codes [w, c] / scales [w, c/256] of ONE chunk from w workers -> requantised sum, rank order."""
    acc = torch.zeros(codes.shape[1])
    for w in range(codes.shape[0]):
        acc = acc + dequant(codes[w], scales[w])
    q, s = quant(acc.view(-1, QB), bits)
    return q.view(1, -1), s.view(1, -1)


def exact_span(n, bits, seed=0):
    """Exact-by-construction values: integers k in [-QMAX, QMAX] times 2^-10, the first element of every
    (possibly partial) block equal to QMAX * 2^-10: codes == k and scales == 2^-10 with every fp32 operation
    exact.  Returns (values fp32 [n], k int8 [n])."""
    q = int(qmax(bits))
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-q, q + 1, (n,), generator=g)
    k[0::QB] = q
    return k.float() * 2.0 ** -10, k.to(torch.int8)


# (L, W): less than one block, one block, a partial last block, and with 3 workers a last chunk that is
# partly / entirely padding (c = 256: chunk 2 holds 188 / 0 real elements), a multi-block 3-worker span, and
# a length that is no multiple of 4 (the last lane's float4 is cut)
SIZES = [(64, 1), (256, 1), (256 * 9 + 64, 1), (700, 3), (300, 3), (256 * 9 + 64, 3), (777, 2)]
