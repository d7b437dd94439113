"""Sentinel frames for kernels that write in place or into views: the operand sits in the middle of a larger
buffer prefilled with a bit pattern that must survive the launch, bit for bit."""
import torch

DEV = "cuda"


def _ints(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# NaN payloads: a stray read shows as well as a stray write.  One-byte elements (fp8, uint8) have no spare NaN
# payload -- e4m3fn has a single NaN per sign, which a quantiser writes for a NaN input -- so their sentinel is
# 0xA5: a finite negative code in both fp8 formats (e4m3 -0.203125, e5m2 -0.01953125).
_PATTERN = {1: 0xA5, 2: 0x7FC1, 4: 0x7FC12345}


def framed(rows, cols, dtype, pad_r=1, pad_c=16):
    """A [rows, cols] view in the middle of a larger buffer prefilled with a sentinel bit pattern."""
    big = torch.empty(rows + 2 * pad_r, cols + 2 * pad_c, dtype=dtype, device=DEV)
    _ints(big).fill_(_PATTERN[big.element_size()])
    return big, big[pad_r:pad_r + rows, pad_c:pad_c + cols]


def framed_flat(n, dtype, pad=16):
    big = torch.empty(n + 2 * pad, dtype=dtype, device=DEV)
    _ints(big).fill_(_PATTERN[big.element_size()])
    return big, big[pad:pad + n]


def assert_frame_intact(big, view=None):
    """Every element of ``big`` outside ``view`` (None: all of it) still holds the sentinel, bit for bit."""
    b = _ints(big).clone()
    off = (view.data_ptr() - big.data_ptr()) // big.element_size() if view is not None else 0
    if view is None:
        pass
    elif big.dim() == 1:
        b[off:off + view.numel()] = _PATTERN[big.element_size()]
    else:
        r0, c0 = off // big.stride(0), off % big.stride(0)
        b[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = _PATTERN[big.element_size()]
    assert bool((b == _PATTERN[big.element_size()]).all()), "a neighbouring element was overwritten"
