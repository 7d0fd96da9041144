"""Fragment addressing of the four-wave GEMM (gemm_q.hip, variant 32), checked exactly.

The asm fragment reads take a per-lane base plus an immediate offset that encodes (operand,
k-sub kk, row tile r) and follow the two LDS stages through the K loop.  A fragment read from
the wrong place is a wrong 16 x 32 block of one operand in one MFMA; under the sqrt(K)
tolerances of test_gemm_q_gpu.py it can hide inside a long K.  Here the operands are
integer-valued bf16 from {-4..4}: every product and every partial sum is an integer of
magnitude <= 16 K < 2^24, exact in fp32 in any summation order, so the result must EQUAL
A.float() @ B.float() (bf16 output: that reference rounded to bf16 once).

Shapes (all four operand layouts each): one tile and one K-tile (256 x 256 x 64: all four
waves); K = 192 (both LDS stages and the wrap back to stage 0); K = 200 (K tail, strided and
contiguous); 264 x 280 x 328 (ragged second tile in both dimensions); the weight-gradient form
split over K into slabs + slab_sum at 512 x 792 x 1024 (the first layer's ragged column tile).
The position-coded cases make every operand row a one-hot pattern with its own power-of-two
scale, so each (row tile, kk) fragment is told apart from its neighbours.
"""
import pytest
import torch

import ldnn  # noqa: F401
from ldnn.ops import _ext

pytestmark = pytest.mark.gpu

LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]
SHAPES = [(256, 256, 64), (256, 256, 192), (256, 256, 200), (264, 280, 328)]

_CASES = {}


def C():
    return _ext.C()


def _case(M, N, K):
    """Logical A [M][K], B [K][N] and the exact fp32 product: made once per shape, never written."""
    if (M, N, K) not in _CASES:
        g = torch.Generator(device="cuda").manual_seed(M * 7 + N * 3 + K)
        A = torch.randint(-4, 5, (M, K), device="cuda", generator=g).bfloat16()
        B = torch.randint(-4, 5, (K, N), device="cuda", generator=g).bfloat16()
        _CASES[(M, N, K)] = (A, B, A.float() @ B.float())
    return _CASES[(M, N, K)]


def _layout(A, B, a_kc, b_kc):
    return (A if a_kc else A.t()).contiguous(), (B.t() if b_kc else B).contiguous()


@pytest.mark.parametrize("out_f32", [True, False])
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_integer_operands_exact(M, N, K, a_kc, b_kc, out_f32):
    A, B, ref = _case(M, N, K)
    a, b = _layout(A, B, a_kc, b_kc)
    if out_f32:
        c = torch.full((M, N), float("nan"), device="cuda")
        want = ref
    else:
        c = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
        want = ref.bfloat16()
    C().gemm(a, b, c, a_kc, b_kc, tile=256, variant=32)
    torch.cuda.synchronize()
    bad = int((c != want).sum().item())
    print(f"{M}x{N}x{K} a_kc={a_kc} b_kc={b_kc} f32={out_f32}: {bad} of {M * N} elements differ")
    assert torch.equal(c, want)


def test_wgrad_split_slabs_exact():
    """dW = dY^T X split over K in two: each slab is exactly its half of the K range, and
    slab_sum of the two is the exact product (N = 792: three full column tiles and 24 columns)."""
    M, N, K = 512, 792, 1024
    A, B, ref = _case(M, N, K)
    a, b = _layout(A, B, False, False)
    slabs = torch.full((2, M, N), float("nan"), device="cuda")
    out = torch.full((M, N), float("nan"), device="cuda")
    C().gemm(a, b, slabs, False, False, tile=256, splitk=2)
    C().slab_sum(slabs, out)
    torch.cuda.synchronize()
    h = K // 2   # 16 K-tiles, 8 per slab
    for s in range(2):
        part = A[:, s * h:(s + 1) * h].float() @ B[s * h:(s + 1) * h].float()
        bad = int((slabs[s] != part).sum().item())
        print(f"slab {s}: {bad} of {M * N} elements differ")
        assert torch.equal(slabs[s], part)
    assert torch.equal(out, ref)


def _coded(rows, K):
    """[rows][K] one-hot rows: row i holds 2^(i // K) at k = i % K -- (position, scale) is distinct
    per row; and a dense [rows][K] pattern of small integers that differs from row to row and
    from k to k (both exact in bf16)."""
    i = torch.arange(rows, device="cuda")
    onehot = torch.zeros(rows, K, device="cuda")
    onehot[i, i % K] = torch.pow(2.0, (i // K).float())
    dense = ((i[:, None] * 13 + torch.arange(K, device="cuda")[None, :] * 7) % 97 + 1).float()
    return onehot.bfloat16(), dense.bfloat16()


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("coded", ["a", "b"])
def test_position_coded_fragments(coded, a_kc, b_kc):
    """One operand one-hot per row with its own scale, the other dense and asymmetric: every
    C[m][n] is a single product, scale(m) * dense[n][m % K] (or the mirror image), so a fragment
    of another row tile, of the other k-sub or of the other stage shows as a wrong value.
    512 x 512 x 128: four tiles, both k-subs of both LDS stages, scales 1, 2, 4, 8."""
    M = N = 512
    K = 128
    onehot, dense = _coded(M, K)
    A, Bt = (onehot, dense) if coded == "a" else (dense, onehot)   # A [M][K], Bt [N][K]
    a, b = _layout(A, Bt.t(), a_kc, b_kc)
    c = torch.full((M, N), float("nan"), device="cuda")
    C().gemm(a, b, c, a_kc, b_kc, tile=256, variant=32)
    torch.cuda.synchronize()
    i = torch.arange(M, device="cuda")
    scale = torch.pow(2.0, (i // K).float())
    if coded == "a":
        want = scale[:, None] * dense.float()[:, i % K].t()      # [m][n] = 2^(m // K) * dense[n][m % K]
    else:
        want = dense.float()[:, i % K] * scale[None, :]          # [m][n] = dense[m][n % K] * 2^(n // K)
    assert torch.equal(want, A.float() @ Bt.float().t())         # the closed form is the product
    bad = int((c != want).sum().item())
    print(f"coded {coded} a_kc={a_kc} b_kc={b_kc}: {bad} of {M * N} elements differ")
    assert torch.equal(c, want)
