"""Strided operands with poisoned padding, for kernel tests.

A kernel that takes a leading dimension makes three promises: nothing outside the
logical [rows][cols] extent of an input influences an output, nothing outside the
logical extent of an output is written, and a base pointer that is 16-B aligned (and
no more) works.  `poisoned` builds operands that make a broken promise visible:

    view, h = poisoned(rows, cols, ld=..., dtype=..., device=..., fill="nan")
    write_inside(view, dense)           # operand data in, padding stays poisoned
    kernel(view, ...)
    assert_no_poison(out_view, "c")     # a read outside an input shows up as NaN
    assert_outside_untouched(out_h)     # a write outside an output breaks the sentinel

All padding is allocated memory (`before` rows in front, `after` rows behind, the
columns left and right of the view), so an over-reading kernel returns poison and
never touches unmapped memory.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

_INT_OF = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32,
           torch.uint8: torch.uint8, torch.int32: torch.int32}
# fixed, finite, unlikely bit patterns for output buffers (bf16 0x4D4D ~ 2.1e8, fp32 0x4D4D4D4D ~ 2.2e8)
_SENTINEL = {torch.bfloat16: 0x4D4D, torch.float16: 0x4D4D, torch.float32: 0x4D4D4D4D, torch.uint8: 0xA5,
             torch.int32: 0x4D4D4D4D}
_NAN = {torch.bfloat16: 0x7FC0, torch.float16: 0x7E00, torch.float32: 0x7FC00000}


@dataclass
class Handle:
    """The whole allocation behind a poisoned view."""
    raw: torch.Tensor      # 1-D, everything allocated (a 16-B lead-in included)
    buf: torch.Tensor      # [before + rows + after][ld], the padded matrix inside `raw`
    view: torch.Tensor     # [rows][cols] at (before, col0) of `buf`
    lead: int              # elements of `raw` in front of `buf`
    before: int
    col0: int
    fill_bits: int


def _fill_bits(dtype, fill):
    if fill == "nan":
        assert dtype in _NAN, f"no NaN in {dtype}: poison it with fill='ff'"
        return _NAN[dtype]
    if fill == "ff":
        return {1: 0xFF, 2: -1, 4: -1}[torch.empty((), dtype=dtype).element_size()]
    if fill == "sentinel":
        return _SENTINEL[dtype]
    if fill == "zero":   # documented zero-padding contracts
        return 0
    raise ValueError(f"fill must be 'nan', 'ff', 'sentinel' or 'zero', got {fill!r}")


def poisoned(rows, cols, *, ld, before=0, after=1, col0=0, dtype=torch.bfloat16, device="cpu", fill="nan",
             aligned=True, full_rows=False):
    """One buffer of (before + rows + after) * ld elements filled with `fill` ('nan' for float
    inputs, 'ff' = all-ones bytes for uint8 masks, 'sentinel' = a fixed finite bit pattern for
    outputs, 'zero' for a documented zero pad); returns its [rows][cols] view at row `before`,
    column `col0`, and the Handle of the allocation.

    `aligned`: the view starts on a 16-B boundary and on no 32-B one (the allocation is
    shifted by 16 B when rows and columns alone would give more), which is the most any
    binding asks for.  Byte masks pass aligned=False.

    `full_rows`: the view spans whole rows (cols == ld, col0 == 0) and only the rows in front and
    behind are padding: for outputs whose kernel writes the pad columns by contract."""
    assert rows >= 1 and cols >= 1 and before >= 0 and after >= 1 and col0 >= 0
    if full_rows:
        assert cols == ld and col0 == 0, "full_rows: cols == ld and col0 == 0"
    else:
        assert ld - cols - col0 > 0, f"no pad columns right of the view: ld {ld}, cols {cols}, col0 {col0}"
    item = torch.empty((), dtype=dtype).element_size()
    n = (before + rows + after) * ld
    off = (before * ld + col0) * item
    lead = 0
    if aligned:
        assert off % 16 == 0, f"view offset {off} B is not 16-B aligned (ld {ld}, before {before}, col0 {col0})"
        lead = (16 // item) if off % 32 == 0 else 0
    bits = _fill_bits(dtype, fill)
    raw = torch.empty(lead + n + 16 // item, dtype=dtype, device=device)
    raw.view(_INT_OF[dtype]).fill_(bits)
    buf = raw[lead:lead + n].view(before + rows + after, ld)
    view = buf[before:before + rows, col0:col0 + cols]
    if aligned:
        assert raw.data_ptr() % 32 == 0, "allocator returned a buffer that is not 32-B aligned"
        assert view.data_ptr() % 16 == 0 and view.data_ptr() % 32 != 0
    return view, Handle(raw, buf, view, lead, before, col0, bits)


def write_inside(view, dense):
    """Copy the operand data into the view; the poison around it stays."""
    assert tuple(view.shape) == tuple(dense.shape), (tuple(view.shape), tuple(dense.shape))
    view.copy_(dense.to(view.dtype))
    return view


def strided_like(dense, *, ld, before=0, after=1, col0=0, fill="nan", aligned=True):
    """poisoned() + write_inside() for a 2-D dense operand."""
    view, h = poisoned(dense.shape[0], dense.shape[1], ld=ld, before=before, after=after, col0=col0,
                       dtype=dense.dtype, device=dense.device, fill=fill, aligned=aligned)
    write_inside(view, dense)
    return view, h


def _coords(bad, limit=5):
    idx = bad.nonzero()[:limit].tolist()
    return ", ".join("(" + ", ".join(str(i) for i in c) + ")" for c in idx), int(bad.sum().item())


def assert_outside_untouched(handle, what="output"):
    """Everything of the allocation outside the view still holds the fill, bit for bit."""
    it = _INT_OF[handle.raw.dtype]
    bits = handle.buf.view(it)
    outside = torch.ones_like(bits, dtype=torch.bool)
    r, c = handle.view.shape
    outside[handle.before:handle.before + r, handle.col0:handle.col0 + c] = False
    bad = (bits != handle.fill_bits) & outside
    if bad.any():
        where, count = _coords(bad)
        raise AssertionError(f"{what}: {count} element(s) outside the [{r}][{c}] view at (row {handle.before}, "
                             f"col {handle.col0}) of the [{bits.shape[0]}][{bits.shape[1]}] buffer were written; "
                             f"first (buffer row, buffer col): {where}")
    rawb = handle.raw.view(it)
    edge = torch.cat([rawb[:handle.lead], rawb[handle.lead + bits.numel():]])
    if (edge != handle.fill_bits).any():
        raise AssertionError(f"{what}: the 16 B in front of or behind the buffer were written")


def assert_no_poison(out_view, what="output"):
    """The output is all finite; a failure names the first few (row, col) of the leak."""
    bad = ~torch.isfinite(out_view.float())
    if bad.any():
        where, count = _coords(bad)
        raise AssertionError(f"{what}: {count} non-finite value(s) of {tuple(out_view.shape)}: padding leaked "
                             f"into the result; first (row, col): {where}")


# ---- the three-step protocol of the strided kernel tests -------------------------------------

class T:
    """One tensor of a kernel call.  `data`: its dense content (inputs, accumulated-into
    outputs) or None (pure outputs, given by shape / dtype).  role: 'in' (NaN padding),
    'mask_in' (0xFF padding), 'out' (sentinel padding; the strided result must equal the dense
    one unless exact=False), 'dense' (dense by the binding's contract: never strided).
    ld / col0 override the padding style; full_rows, aligned: see poisoned()."""

    def __init__(self, role, data=None, shape=None, dtype=None, exact=True, ld=None, col0=0, full_rows=False,
                 aligned=None):
        self.role, self.data, self.exact = role, data, exact
        self.shape = tuple(data.shape) if data is not None else tuple(shape)
        self.dtype = data.dtype if data is not None else dtype
        self.ld, self.col0, self.full_rows = ld, col0, full_rows
        # 16-B (and no more) aligned unless the binding asks for no alignment of this operand
        self.aligned = (self.dtype != torch.uint8) if aligned is None else aligned


def padded_ld(cols, style, item):
    """(ld, col0) of a padding style.  'min': cols + 8 elements, the least a binding allows, no left
    pad; 'eng': cols rounded up to 64 plus 64, the engine's style, and 16 B of left pad."""
    if style == "min":
        return cols + 8, 0
    return (cols + 63) // 64 * 64 + 64, 16 // item


def _sentinel_dense(shape, dtype, device):
    t = torch.empty(shape, dtype=dtype, device=device)
    t.view(_INT_OF[dtype]).fill_(_SENTINEL[dtype])
    return t


def materialize(spec, strided, style, before, after, device):
    """name -> T  =>  (name -> tensor for the call, name -> Handle of the strided ones)"""
    ts, hs = {}, {}
    for name, t in spec.items():
        if not strided or t.role == "dense":
            ts[name] = t.data.clone() if t.data is not None else _sentinel_dense(t.shape, t.dtype, device)
            continue
        one_d = len(t.shape) == 1
        rows, cols = (1, t.shape[0]) if one_d else t.shape
        item = torch.empty((), dtype=t.dtype).element_size()
        if t.full_rows:
            ld, col0 = cols, 0
        elif t.ld is not None:
            ld, col0 = t.ld, t.col0
        elif t.dtype == torch.uint8:   # bit masks: byte addressed, any row stride > cols
            ld, col0 = (cols + 3, 0) if style == "min" else (cols + 16, 1)
        else:
            ld, col0 = padded_ld(cols, style, item)
        fill = {"in": "nan", "mask_in": "ff", "out": "sentinel"}[t.role]
        v, h = poisoned(rows, cols, ld=ld, before=0 if one_d else before, after=1 if one_d else after, col0=col0, dtype=t.dtype,
                        device=device, fill=fill, aligned=t.aligned, full_rows=t.full_rows)
        if t.data is not None:
            write_inside(v, t.data.reshape(rows, cols))
        ts[name] = v[0] if one_d else v
        hs[name] = h
    return ts, hs


def three_steps(spec, call, check, style, before, after=256, device="cuda"):
    """1. call(tensors) on dense copies, check(tensors) asserts the bounds against the reference;
    2. the same on poisoned strided views (16-B aligned and no more): no NaN in any output, the
       same bounds, every buffer's padding intact bit for bit;
    3. every output that is not marked exact=False: strided == dense, bit for bit.
    Returns (dense tensors, strided tensors)."""
    def sync():
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()

    dense, _ = materialize(spec, False, style, before, after, device)
    call(dense)
    sync()
    check(dense)
    st, hs = materialize(spec, True, style, before, after, device)
    for name, t in st.items():
        if name in hs and spec[name].aligned and t.dim() == 2:
            assert t.data_ptr() % 16 == 0 and t.data_ptr() % 32 != 0, name
    call(st)
    sync()
    outs = [n for n, t in spec.items() if t.role in ("out", "dense")]
    for n in outs:
        if spec[n].dtype.is_floating_point:
            assert_no_poison(st[n], n)
    check(st)
    for n, h in hs.items():          # outputs keep their sentinel, inputs their poison
        assert_outside_untouched(h, n)
    for n in outs:
        if spec[n].exact:
            assert torch.equal(st[n], dense[n]), f"{n}: the strided result differs from the dense one"
    return dense, st
