"""tests/strided.py does what the strided-operand GPU tests rely on: with torch CPU ops in
place of kernels, a correct matmul on poisoned views passes all three checks, a read of one
column / one row too many fails assert_no_poison, and a write one element past the view
fails assert_outside_untouched."""
import pytest
import torch

from strided import Handle, assert_no_poison, assert_outside_untouched, poisoned, strided_like, write_inside

DTYPES = [torch.bfloat16, torch.float32]
M, N, K = 5, 8, 16


def _operands(dtype, before=0):
    """A [M][K], B [K][N] (both strided, NaN padding) and a sentinel-filled strided C [M][N]."""
    g = torch.Generator().manual_seed(0)
    a_d = torch.randn(M, K, generator=g).to(dtype)
    b_d = torch.randn(K, N, generator=g).to(dtype)
    a, ha = strided_like(a_d, ld=K + 8, before=before)
    b, hb = strided_like(b_d, ld=N + 8, before=before)
    c, hc = poisoned(M, N, ld=N + 8, before=before, dtype=dtype, fill="sentinel")
    return a_d, b_d, a, ha, b, hb, c, hc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("before", [0, 3])
def test_view_geometry_and_alignment(dtype, before):
    v, h = poisoned(M, N, ld=N + 8, before=before, after=2, dtype=dtype, fill="nan")
    assert isinstance(h, Handle) and v.shape == (M, N) and v.stride() == (N + 8, 1)
    assert v.data_ptr() % 16 == 0 and v.data_ptr() % 32 != 0
    assert h.buf.shape == (before + M + 2, N + 8)
    assert torch.isnan(h.raw.float()).all()                 # all of it is poison before write_inside
    write_inside(v, torch.ones(M, N))
    assert torch.isfinite(v.float()).all() and int(torch.isnan(h.buf.float()).sum()) == h.buf.numel() - M * N
    # a left pad (col0 > 0) keeps the 16-B alignment too
    v2, _ = poisoned(M, N, ld=N + 24, col0=8, dtype=dtype)
    assert v2.data_ptr() % 16 == 0 and v2.data_ptr() % 32 != 0
    with pytest.raises(AssertionError, match="no pad columns"):
        poisoned(M, N, ld=N + 8, col0=8, dtype=dtype)
    with pytest.raises(AssertionError, match="not 16-B aligned"):
        poisoned(M, N, ld=N + 8, col0=1, dtype=dtype)


def test_byte_mask_poison():
    v, h = poisoned(4, 3, ld=5, col0=1, dtype=torch.uint8, fill="ff", aligned=False)
    assert int(h.raw.min()) == 0xFF
    v.zero_()
    assert_outside_untouched(h, "mask")
    h.buf[2, 4] = 0
    with pytest.raises(AssertionError, match=r"mask: 1 element\(s\) outside .*\(2, 4\)"):
        assert_outside_untouched(h, "mask")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("before", [0, 3])
def test_correct_matmul_passes(dtype, before):
    a_d, b_d, a, ha, b, hb, c, hc = _operands(dtype, before)
    c.copy_(a @ b)
    assert_no_poison(c, "c")
    assert torch.equal(c, a_d @ b_d)                        # the leading dimension changes nothing
    ref = a_d.double() @ b_d.double()
    assert (c.double() - ref).abs().max().item() <= 2 ** -7 * ref.abs().max().item()
    for h in (ha, hb, hc):
        assert_outside_untouched(h)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reading_one_column_too_many_is_caught(dtype):
    """A K loop that runs one element into A's pad columns (and B's pad row)."""
    _, _, a, ha, b, hb, c, hc = _operands(dtype)
    a_over = ha.buf[:M, :K + 1]
    b_over = hb.buf[:K + 1, :N]
    c.copy_(a_over @ b_over)
    with pytest.raises(AssertionError, match=r"c: 40 non-finite value\(s\).*first \(row, col\): \(0, 0\)"):
        assert_no_poison(c, "c")


@pytest.mark.parametrize("dtype", DTYPES)
def test_reading_one_row_too_many_is_caught(dtype):
    """A column sum (a bias gradient) that takes in the first pad row behind the operand: with
    before=3 the same over-read in front of it."""
    _, _, a, ha, _, _, _, _ = _operands(dtype, before=3)
    good = a.float().sum(0)
    assert_no_poison(good, "dbias")
    behind = ha.buf[3:3 + M + 1, :K].float().sum(0)
    with pytest.raises(AssertionError, match=r"dbias: 16 non-finite"):
        assert_no_poison(behind, "dbias")
    front = ha.buf[2:3 + M, :K].float().sum(0)
    with pytest.raises(AssertionError, match=r"dbias: 16 non-finite"):
        assert_no_poison(front, "dbias")
    # a leak into one output column names that column
    leak = good.clone()
    leak[11] += ha.buf[3 + M, 11].float()
    with pytest.raises(AssertionError, match=r"first \(row, col\): \(11\)"):
        assert_no_poison(leak, "dbias")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("before", [0, 3])
def test_writing_one_element_past_the_view_is_caught(dtype, before):
    a_d, b_d, a, _, b, _, c, hc = _operands(dtype, before)
    c.copy_(a @ b)
    assert_outside_untouched(hc, "c")
    # one element right of the last row's last column
    hc.buf[before + M - 1, N] = 1.0
    with pytest.raises(AssertionError, match=rf"c: 1 element\(s\) outside .*\({before + M - 1}, {N}\)"):
        assert_outside_untouched(hc, "c")
    # one row below, first column (a row tail that is stored unmasked)
    _, _, _, _, _, _, c2, hc2 = _operands(dtype, before)
    hc2.buf[before + M, 0] = 0.0
    with pytest.raises(AssertionError, match=rf"\({before + M}, 0\)"):
        assert_outside_untouched(hc2, "c")
    # the 16 B in front of the whole buffer (an under-run of a view at row 0)
    _, _, _, _, _, _, c3, hc3 = _operands(dtype, before)
    if hc3.lead:
        hc3.raw[hc3.lead - 1] = 0.0
        with pytest.raises(AssertionError, match="in front of or behind"):
            assert_outside_untouched(hc3, "c")


@pytest.mark.parametrize("dtype", DTYPES)
def test_rewriting_the_sentinel_bits_outside_is_not_a_false_alarm_but_any_other_bits_are(dtype):
    """The comparison is on bits: -0.0 over a 0-fill differs, NaN over NaN poison does not."""
    v, h = poisoned(M, N, ld=N + 8, dtype=dtype, fill="zero")
    assert_outside_untouched(h)
    h.buf[0, N] = -0.0
    with pytest.raises(AssertionError, match=rf"\(0, {N}\)"):
        assert_outside_untouched(h)
    v, h = poisoned(M, N, ld=N + 8, dtype=dtype, fill="nan")
    h.buf[0, N] = float("nan")
    assert_outside_untouched(h)
