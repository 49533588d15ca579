"""CPU: tests/footprint.py can fail.  Fake "kernels" written with torch ops on CPU windows: one stores an element before the window,
one behind it, one a whole extra row, one sums a row too many of a 0xff-margined input (NaN reaches the result); each is reported
with the right offset, and the correct kernel passes.  Alignment and margin sizes for fp32, bf16, uint8 and 24-bit rows."""
import pytest
import torch

import footprint as F

CPU = torch.device("cpu")
ROWS, WIDTH = 5, 256


def _flat(w, dtype):
    """The whole allocation as `dtype` elements, and the index of the window's first element in it (what a kernel with a wrong
    index addresses)."""
    item = torch.empty((), dtype=dtype).element_size()
    assert w.start % item == 0
    n = w.base.numel() // item * item
    return w.base[:n].view(dtype), w.start // item


def _kernel(out_w, in_w, rows, first_row=0, extra_rows=0, element_before=False, element_behind=False):
    """y[r] = 2 x[r] for `rows` rows -- with the defects the tests ask for, all of them through flat indices as a kernel would."""
    width = in_w.view.shape[1]
    xs, x0 = _flat(in_w, torch.float32)
    ys, y0 = _flat(out_w, torch.float32)
    n = (rows + extra_rows) * width
    ys[y0 + first_row * width:y0 + first_row * width + n] = 2 * xs[x0:x0 + n]
    if element_before:
        ys[y0 - 1] = 1.0
    if element_behind:
        ys[y0 + rows * width] = 1.0


def _case():
    x = torch.randn(ROWS, WIDTH, generator=torch.Generator().manual_seed(0))
    return x, F.window((ROWS, WIDTH), torch.float32, CPU, F.POISON, body=x, what="x"), \
        F.window((ROWS, WIDTH), torch.float32, CPU, F.GUARD, what="y")


def test_correct_kernel_passes():
    x, xw, yw = _case()
    _kernel(yw, xw, ROWS)
    assert xw.margins_intact() and yw.margins_intact()
    assert yw.margin_damage() is None
    assert F.same_bits(yw.view, 2 * x)
    assert F.same_bits(xw.view, x)


def test_store_before_the_window_is_reported():
    _, xw, yw = _case()
    _kernel(yw, xw, ROWS, element_before=True)
    assert yw.margin_damage() == -4                 # 1.0f = 00 00 80 3f: all four bytes differ from 0xa5, the first is at -4
    with pytest.raises(AssertionError, match=r"offset -4 .*before the window"):
        yw.margins_intact()
    assert xw.margins_intact()


def test_store_behind_the_window_is_reported():
    _, xw, yw = _case()
    _kernel(yw, xw, ROWS, element_behind=True)
    assert yw.margin_damage() == ROWS * WIDTH * 4
    with pytest.raises(AssertionError, match=rf"offset {ROWS * WIDTH * 4} .*0 bytes behind its end"):
        yw.margins_intact()


def test_extra_row_is_reported():
    """One row too many: the input's margin is NaN, so the row behind the output holds NaN bits (0xffffffff) instead of 0xa5."""
    _, xw, yw = _case()
    _kernel(yw, xw, ROWS, extra_rows=1)
    assert yw.margin_damage() == ROWS * WIDTH * 4
    assert xw.margins_intact()                      # reading changes nothing
    # ... and all of that row, no more: the byte behind it is intact
    back = yw.base[yw.start + yw.nbytes:]
    assert bool((back[:WIDTH * 4] != F.GUARD).all()) and F.all_bytes(back[WIDTH * 4:], F.GUARD)


def test_unwritten_output_rows_keep_the_guard():
    """A3: an output with pad rows the contract leaves alone -- a kernel that fills them is caught by the body check."""
    x, xw, _ = _case()
    yw = F.window((F.ceil256(ROWS), WIDTH), torch.float32, CPU, F.GUARD, what="y")
    _kernel(yw, xw, ROWS)
    assert F.all_bytes(yw.view[ROWS:], F.GUARD)
    _kernel(yw, xw, ROWS, extra_rows=1)
    with pytest.raises(AssertionError, match="offset 0 "):
        F.all_bytes(yw.view[ROWS:], F.GUARD)
    assert yw.margins_intact()                      # the store stayed inside the window: only A3 sees it


def test_row_too_many_of_a_poisoned_input_reaches_the_result():
    """A1: a column sum over rows + 1 rows reads the 0xff margin: NaN, where the plain call's sum is finite."""
    x, xw, _ = _case()
    xs, x0 = _flat(xw, torch.float32)
    good = xs[x0:x0 + ROWS * WIDTH].view(ROWS, WIDTH).sum(0)
    bad = xs[x0:x0 + (ROWS + 1) * WIDTH].view(ROWS + 1, WIDTH).sum(0)
    assert F.same_bits(good, x.sum(0))
    assert torch.isnan(bad).all()
    with pytest.raises(AssertionError, match="bits differ: first at byte "):
        F.same_bits(bad, x.sum(0))
    # the same through pad rows: a ceil256-row operand whose pad rows are poisoned
    a = torch.zeros(F.ceil256(ROWS), WIDTH)
    a[:ROWS] = x
    F.poison_pad_rows(a, ROWS)
    assert F.same_bits(a[:ROWS], x) and torch.isnan(a[ROWS:]).all() and F.all_bytes(a[ROWS:], F.POISON)
    assert torch.isnan(a[:ROWS + 1].sum(0)).all()


def test_int_poison_is_loud():
    ids = torch.tensor([[3, 9, 4], [7, 1, 2]], dtype=torch.int32)
    w = F.window(ids.shape, torch.int32, CPU, F.INT_POISON, body=ids, what="ids")
    flat, i0 = _flat(w, torch.int32)
    assert int(flat[i0 - 1]) == F.INT_POISON and int(flat[i0 + 6]) == F.INT_POISON
    assert int(flat[i0:i0 + 6].view(2, 3).argmax(-1)[1]) == 0
    assert int(flat[i0 + 3:i0 + 7].argmax()) == 3   # an arg-max over one element too many picks the margin
    assert w.margins_intact()
    flat[i0 + 6] = 5
    assert w.margin_damage() == 24
    w2 = F.window((4,), torch.int32, CPU, F.INT_POISON, what="idx")
    assert torch.equal(w2.view, torch.full((4,), F.INT_POISON, dtype=torch.int32))
    with pytest.raises(AssertionError):
        F.window((3,), torch.uint8, CPU, F.INT_POISON)


@pytest.mark.parametrize("dtype,shape,row_bytes", [
    (torch.float32, (5, 256), 1024), (torch.float32, (133, 1280), 5120), (torch.bfloat16, (5, 768), 1536),
    (torch.bfloat16, (300, 3840), 7680), (torch.uint8, (1000,), 1), (torch.uint8, (5, 3 * 256), 768),      # 24-bit rows: 3 W bytes
    (torch.uint8, (133, 3 * 1280), 3840), (torch.int32, (7,), 4), (torch.float8_e4m3fn, (300, 256), 256)])
def test_alignment_and_margin_sizes(dtype, shape, row_bytes):
    w = F.window(shape, dtype, CPU, F.GUARD)
    assert w.view.dtype == dtype and tuple(w.view.shape) == shape
    assert w.ptr % 256 == 0 and w.ptr == w.base.data_ptr() + w.start
    want = max(64 * 1024, 256 * row_bytes)
    assert w.margin == want
    assert w.start >= want and w.base.numel() - (w.start + w.nbytes) >= want      # at least the margin on either side
    assert F.all_bytes(w.base, F.GUARD) and w.margins_intact()
    w.view.view(torch.uint8).fill_(0)                                             # writing the whole body touches no margin
    assert w.margins_intact() and int((w.base == 0).sum()) == w.nbytes
    # every margin byte counts: the first and the last byte of the allocation, and the bytes next to the window
    for pos in (0, w.start - 1, w.start + w.nbytes, w.base.numel() - 1):
        keep = int(w.base[pos])
        w.base[pos] = 0
        assert w.margin_damage() == pos - w.start
        w.base[pos] = keep
    assert w.margins_intact()


def test_row_bytes_override_and_body_forms():
    w = F.window((4096,), torch.uint8, CPU, F.GUARD, body=F.POISON, row_bytes=3 * 1280 * 2, what="workspace")
    assert w.margin == 256 * 3 * 1280 * 2
    assert F.all_bytes(w.view, F.POISON) and w.margins_intact()
    x = torch.arange(12, dtype=torch.float32).view(3, 4)
    assert F.same_bits(F.window((3, 4), torch.float32, CPU, F.POISON, body=x).view, x)
    assert F.same_bits(F.window((3, 4), torch.int32, CPU, F.POISON, body=x).view, x)        # same element size: taken by its bits


# ---- the two-call harness (run_both): A1 / A2 / A3 on a fake kernel that takes tensors
def _fake(defect):
    def kernel(x, y, rows):
        """y[r] = x[r] + x[r + 1] for r < rows (x has ceil256(rows) rows: row `rows` is a pad row the correct kernel masks out)."""
        xs = x[:rows + 1].clone()
        if defect != "reads_pad_row":
            xs[rows] = 0
        y[:rows] = xs[:rows] + xs[1:rows + 1]
        if defect == "writes_pad_row":
            y[rows] = 0
        if defect == "writes_behind":
            try:                                          # one element past the buffer the kernel was given
                torch.as_strided(y.view(-1), (y.numel() + 1,), (1,))[-1] = 1.0
            except RuntimeError:                          # (the plain call's tight tensor: torch refuses what a GPU would not)
                pass
    return kernel


def _fake_specs(rows=5, width=8):
    x = torch.zeros(F.ceil256(rows), width)
    x[:rows] = torch.randn(rows, width, generator=torch.Generator().manual_seed(1))
    return [F.In(x, valid_rows=rows), F.Out((F.ceil256(rows), width), torch.float32, written=lambda v: v[:rows], keep=lambda v: v[rows:]), rows]


def test_run_both_passes_a_correct_kernel_and_names_each_defect():
    calls = F.run_both(_fake(None), _fake_specs(), CPU, as_arg=lambda t: t)
    assert F.same_bits(calls.win[1].view[:5], calls.plain[1][:5]) and F.all_bytes(calls.win[1].view[5:], F.GUARD)
    with pytest.raises(AssertionError, match="contract call != plain call"):       # A1: the poisoned pad row reached row 4
        F.run_both(_fake("reads_pad_row"), _fake_specs(), CPU, as_arg=lambda t: t)
    with pytest.raises(AssertionError, match="bytes the contract leaves alone were written"):      # A3
        F.run_both(_fake("writes_pad_row"), _fake_specs(), CPU, as_arg=lambda t: t)
    with pytest.raises(AssertionError, match=rf"margin byte at offset {256 * 8 * 4} "):            # A2
        F.run_both(_fake("writes_behind"), _fake_specs(), CPU, as_arg=lambda t: t)


def test_run_both_workspace_and_read_modify_write():
    def kernel(ws, c, n):
        ws[:n] = 1                                        # scratch: written before it is read
        c[:n] += ws[:n].float()
    c0 = torch.arange(8, dtype=torch.float32)
    calls = F.run_both(kernel, [F.Work(16, plain_bytes=64), F.Out((8,), torch.float32, init=c0, keep=lambda v: v[4:]), 4], CPU, as_arg=lambda t: t)
    assert calls.win[0].nbytes == 16 and calls.plain[0].numel() == 256 and int(calls.plain[0].sum()) == 4
    assert torch.equal(calls.win[1].view, c0 + torch.tensor([1.0] * 4 + [0.0] * 4))
    with pytest.raises(AssertionError, match="leaves alone"):
        F.run_both(lambda ws, c, n: c.add_(1), [F.Work(16), F.Out((8,), torch.float32, init=c0, keep=lambda v: v[4:]), 4], CPU, as_arg=lambda t: t)
    with pytest.raises(AssertionError, match="contract call != plain call"):   # a result that depends on workspace bytes it never wrote
        F.run_both(lambda ws, c, n: c.add_(ws[:8].float()), [F.Work(16), F.Out((8,), torch.float32, init=c0), 4], CPU, as_arg=lambda t: t)
