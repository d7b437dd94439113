"""tests/_gemm_exact.py on the CPU: the generators stay inside their bound, fp32 arithmetic on them is exact, the
epilogue-isolating inputs survive the bf16 round trip, every epilogue oracle agrees with its fp32 twin (and with
ops/reference.py where it has one), and ``expect_bits`` sees one flipped low bit and names its tile."""
import pytest
import torch

from nanodiloco_amd.ops import reference as ref

from . import _gemm_exact as X
from . import _oracle64 as o64

E4, E5 = X.E4, X.E5


@pytest.mark.parametrize("dtype", [torch.bfloat16, E4, E5], ids=["bf16", "e4m3", "e5m2"])
@pytest.mark.parametrize("K", [64, 2624, 5248])
def test_generators_stay_inside_the_bound_and_fp32_is_exact(dtype, K):
    a = X.int_operand(37, K, -8, 8, dtype, 1)
    b = X.int_operand(24, K, -8, 8, E4 if dtype != torch.bfloat16 else dtype, 2)
    assert a.dtype == dtype and a.float().abs().max().item() <= 8 and torch.equal(a.float(), a.float().round())
    bound = X.exact_bound(K, 8, 8)
    assert bound < X.EXACT_LIMIT
    # the bound holds for the worst partial sum: sum |a_k b_k| over all k
    assert (a.float().abs().double() @ b.float().abs().double().t()).max().item() <= bound
    ex = X.exact_nt(a, b)
    assert torch.equal((a.float() @ b.float().t()).double(), ex)  # fp32 matmul, any order: exact
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(3))
    assert torch.equal((a.float()[:, perm] @ b.float()[:, perm].t()).double(), ex)
    assert X.exact_bound(262143, 8, 8) < X.EXACT_LIMIT <= X.exact_bound(262144, 8, 8)


def test_most_bf16_outputs_need_rounding():
    """K = 2624, values in [-8, 8]: most exact products have more than 8 significant bits, so the rounding mode of
    the bf16 store is tested on most elements, and truncation differs from round-to-nearest-even on many."""
    a = X.int_operand(128, 2624, -8, 8, torch.bfloat16, 1)
    b = X.int_operand(128, 2624, -8, 8, torch.bfloat16, 2)
    ex = X.exact_nt(a, b)
    rne = X.to_dtype(ex, torch.bfloat16)
    assert (rne.double() != ex).float().mean().item() > 0.5
    trunc = (ex.float().view(torch.int32) & -65536).view(torch.float32)  # drop the low 16 bits
    msg = X.describe_mismatch(trunc.bfloat16(), ex)
    assert msg is not None and "elements differ" in msg


def test_exact_tn_with_integer_initial_value():
    K, M, N = 777, 24, 40
    dy = X.int_operand(K, M, -8, 8, torch.bfloat16, 4)
    x = X.int_operand(K, N, -8, 8, torch.bfloat16, 5)
    gw0 = X.int_operand(M, N, -1000, 1000, torch.float32, 6)
    assert X.exact_bound(K, 8, 8, 1000) < X.EXACT_LIMIT
    ex = X.exact_tn(dy, x, gw0)
    assert torch.equal((gw0 + dy.float().t() @ x.float()).double(), ex)
    assert torch.equal(X.exact_tn(dy, x, gw0, scale=0.25), gw0.double() + 0.25 * (ex - gw0.double()))


@pytest.mark.parametrize("K", [64, 128, 256])
@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
def test_iso_operands_survive_bf16(K, f8):
    x, w, sa, sb = X.iso_operands(300, 272, K, 7, f8=f8)
    sc = 1.0 if not f8 else float(sa) * float(sb)
    ex = X.exact_nt(x, w, sc)
    assert torch.equal(ex * 16, (ex * 16).round()) and ex.abs().max().item() <= 16
    assert torch.equal(ex.float().bfloat16().double(), ex)  # the rounding before the epilogue is the identity
    assert torch.equal(((x.float() @ w.float().t()) * sc).double(), ex)
    if not f8:  # the same values in both forms
        x8, w8, sa8, sb8 = X.iso_operands(300, 272, K, 7, f8=True)
        assert torch.equal(X.exact_nt(x8, w8, float(sa8) * float(sb8)), ex)
    # a useful sigmoid range: not all saturated, not all near 0
    assert 1.0 < ex.abs().max().item() and 0.2 < ex.std().item() < 1.0


def test_rope_oracle_agrees_with_twin_and_reference():
    T, hd, B, rc, N = 24, 32, 3, 192, 328
    ex = X.exact_nt(*X.iso_operands(B * T, N, 128, 8)[:2])
    cos, sin = ref.rope_tables(T, hd, 10000.0)
    r64 = X.rope(ex, cos, sin, T, hd, rc)
    tw = X.rope_twin(ex, cos, sin, T, hd, rc)
    assert (tw.double() - r64).abs().max().item() < 1e-5
    assert torch.equal(r64[:, rc:], ex[:, rc:])
    # ops/reference.py: [B, H, T, hd] heads, tables [T, hd]
    heads = ex[:, :rc].float().reshape(B, T, rc // hd, hd).transpose(1, 2)
    rr = ref.apply_rope(heads, cos, sin).transpose(1, 2).reshape(B * T, rc)
    assert (rr.double() - r64[:, :rc]).abs().max().item() < 1e-5
    assert (r64[T:2 * T] - X.rope(ex[T:2 * T], cos, sin, T, hd, rc)).abs().max().item() == 0  # t = row % T


def test_swiglu_oracles_agree_with_twins_and_reference():
    M, F = 129, 136
    gu = X.exact_nt(*X.iso_operands(M, 2 * F, 256, 9)[:2]).float().bfloat16()
    act = X.swiglu_act(gu)
    assert (X.swiglu_act_twin(gu).double() - act).abs().max().item() < 1e-5
    assert (ref.swiglu(gu.float()).double() - act).abs().max().item() < 1e-5
    cf = X.swiglu_coef(gu)
    assert (X.swiglu_coef_twin(gu).double() - cf).abs().max().item() < 1e-5
    d = X.exact_nt(*X.iso_operands(M, F, 64, 10)[:2])
    b0 = X.dswiglu(d, gu, 0)
    assert (X.dswiglu_twin(d, gu, 0).double() - b0).abs().max().item() < 1e-4
    assert (ref.swiglu_backward(d.float(), gu.float()).double() - b0).abs().max().item() < 1e-4
    # form 1 on the unrounded coefficients is form 0
    assert (torch.cat([d, d], 1) * cf - b0).abs().max().item() < 1e-12
    cfb = cf.float().bfloat16()
    b1 = X.dswiglu(d, cfb, 1)
    assert (X.dswiglu_twin(d, cfb, 1).double() - b1).abs().max().item() < 1e-5
    assert torch.equal(b1, torch.cat([d, d], 1) * cfb.double())
    assert torch.equal(b0, o64.swiglu_bwd(d, gu))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_expect_bits_flags_one_flipped_low_bit_and_names_its_tile(dtype):
    ex = X.exact_nt(X.int_operand(300, 64, -8, 8, torch.bfloat16, 11), X.int_operand(520, 64, -8, 8, torch.bfloat16, 12))
    out = X.to_dtype(ex, dtype)
    X.expect_bits(out, ex, "clean")
    assert X.describe_mismatch(out, ex) is None
    bad = out.clone()
    iv = bad.view(torch.int32 if dtype == torch.float32 else torch.int16)
    iv[273, 300] ^= 1
    msg = X.describe_mismatch(bad, ex)
    assert "1 of 156000 elements" in msg and "first at (273, 300)" in msg, msg
    assert "tiles (1, 1)..(1, 1)" in msg, msg
    assert "rows: all = 1 mod 16, all = 17 mod 64, all = 17 mod 128" in msg, msg
    assert "columns: all = 12 mod 16, all = 44 mod 64, all = 44 mod 128" in msg, msg
    with pytest.raises(AssertionError, match="flip: 1 of 156000"):
        X.expect_bits(bad, ex, "flip")
    # a whole wave's column block in one tile: the residue line points at it
    blk = out.clone()
    blk[256:300, 64:128] = 0
    msg = X.describe_mismatch(blk, ex)
    assert "bad rows 256..299, columns 64..127" in msg and "tiles (1, 0)..(1, 0)" in msg, msg
