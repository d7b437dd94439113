"""Inputs of the fp8 KV-cache tests: the rows at which the quantiser (``ops.decode.kv8_quantize``, csrc/attn_kv8.hip)
can go wrong, and a float64 statement of the format that involves neither a float8 dtype nor ``frexp``."""
import torch

from . import _oracle64 as o64


def edge_rows(hd, device="cpu"):
    """bf16 [7, hd]: an all-zero row; amax exactly 1.75 * 2^3 (the last amax of its exponent) and the next bf16 above
    it (the first of the next); a row scaled by 2^0 whose values 17, 19, -21 lie exactly halfway between two codes;
    amax far below the lower clamp (every code 0); amax just below it, with 2^-110 -> 2^-10: half the smallest
    subnormal code, a tie that goes to zero; and a row of one sign with a lone large value."""
    g = torch.Generator().manual_seed(hd)
    x = (torch.randn(7, hd, generator=g) * 2.0).clamp(-6.0, 6.0)
    x[0] = 0.0
    x[1, 3], x[2, hd - 2] = 14.0, -14.0625
    x[3, 0], x[3, 1], x[3, 2], x[3, 3] = 448.0, 17.0, 19.0, -21.0
    x[4] = 0.0
    x[4, 5], x[4, 6] = 2.0 ** -120, -(2.0 ** -124)
    x[5] = 0.0
    x[5, 1], x[5, 2], x[5, 3], x[5, 4] = 1.5 * 2.0 ** -105, 2.0 ** -108, -(2.0 ** -110), 3 * 2.0 ** -110
    x[6] = x[6].abs() * 2.0 ** -6
    x[6, hd - 1] = 300.0
    return x.bfloat16().to(device)


def quantize64(rows):
    """(codes uint8, exps int8) of ``rows`` [n, hd] by search in float64: the exponent is the smallest e in
    [-100, 100] with amax * 2^-e <= 448 (0 for a zero row); the code is the nearest finite e4m3 value of the row's
    sign, ties to the even code, among the 127 magnitudes of ``_oracle64.fp8_codes``."""
    x = rows.double().cpu()
    table = o64.fp8_codes(0)[:127]  # 0 .. 448, increasing; byte 0x7f is NaN
    codes, exps = [], []
    for r in x:
        amax = float(r.abs().max())
        e = 0 if amax == 0 else next((c for c in range(-100, 101) if amax * 2.0 ** -c <= 448.0), 100)
        y = r * 2.0 ** -e  # exact
        d = (y.abs().clamp(max=448.0)[:, None] - table[None]).abs()
        best = d == d.min(-1, keepdim=True).values  # one code, or the two neighbours of a tie
        even = best & (torch.arange(127) % 2 == 0)
        code = torch.where(even.any(-1), even.int().argmax(-1), best.int().argmax(-1))
        codes.append((code | (torch.signbit(y).long() << 7)).to(torch.uint8))
        exps.append(e)
    return torch.stack(codes), torch.tensor(exps, dtype=torch.int8)
