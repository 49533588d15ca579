"""Memory-contract windows for the kernel tests (tests/test_footprint_*.py; DESIGN.md "Memory contracts").

The numerics tests hand the library tight tensors that torch allocated one by one, so a store one row past `m`, or a result that
depends on a pad row the call never wrote, lands in (or reads) whatever torch put next door and passes every rounding budget.  Here
every argument of a call is a WINDOW: a view into one uint8 allocation of the test's own, 256-byte aligned like the library's
buffers, with a margin in front of it and behind it that holds a known byte.

Margin on each side: max(64 KiB, 256 rows of the buffer's widest row).  256 rows is the largest tile any kernel of the library owns
(the 256 x 256 GEMM tiles, the ceil256 pad rows of every operand), so a store or a load that is one whole tile off still lands inside
the test's own allocation: it shows up as a failed assertion, not as damage to somebody else's memory.

Two poison bytes:
  POISON 0xff   "must not reach a result": NaN as fp32, bf16 and e4m3, -1 as int32.  Input margins, input pad rows, workspaces.
  GUARD  0xa5   "must not be written": output margins and the bytes of an output the header says a call leaves alone.
Integer inputs whose stray values must be loud (token ids, pool_idx, row_start, candidate ids) take INT_POISON = 0x7fffffff as an
int32 pattern instead: an arg-max or an index that strays into the margin then changes the answer.

Works on CPU and GPU tensors alike (tests/test_footprint_host.py runs the helper against deliberately wrong torch "kernels").
"""
import torch

ALIGN = 256
MIN_MARGIN = 64 * 1024
TILE_ROWS = 256
POISON = 0xff
GUARD = 0xa5
INT_POISON = 0x7fffffff


def ceil256(n):
    return (n + 255) // 256 * 256


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _pattern(fill, nbytes, device):
    """`nbytes` bytes of the margin pattern, phase 0 (every margin starts at a multiple of 4 bytes from the base)."""
    if fill == INT_POISON:
        assert nbytes % 4 == 0
        return torch.tensor([0xff, 0xff, 0xff, 0x7f], dtype=torch.uint8, device=device).repeat(nbytes // 4)
    assert 0 <= fill <= 255, fill
    return torch.full((nbytes,), fill, dtype=torch.uint8, device=device)


class Window:
    """`view`: the tensor a kernel gets (shape / dtype as asked, first byte 256-byte aligned).  `base`: the one uint8 allocation it
    lives in -- front margin, body, back margin.  Offsets are bytes relative to the window's first byte: negative = front margin,
    >= nbytes = back margin."""

    def __init__(self, base, view, start, nbytes, margin, fill, what):
        self.base, self.view, self.start, self.nbytes, self.margin, self.fill, self.what = base, view, start, nbytes, margin, fill, what

    @property
    def ptr(self):
        return self.view.data_ptr()

    def body_bytes(self):
        return self.base[self.start:self.start + self.nbytes]

    def margin_damage(self):
        """None, or the offset (relative to the window) of the first margin byte that no longer holds the fill."""
        for lo, hi in ((0, self.start), (self.start + self.nbytes, self.base.numel())):
            part = self.base[lo:hi]
            bad = (part != _pattern(self.fill, hi - lo, part.device)).nonzero()
            if bad.numel():
                return lo + int(bad[0]) - self.start
        return None

    def margins_intact(self):
        off = self.margin_damage()
        assert off is None, (f"{self.what}: margin byte at offset {off} of a {self.nbytes}-byte window changed "
                             f"({'before the window' if off < 0 else f'{off - self.nbytes} bytes behind its end'})")
        return True

    def refill_body(self, byte):
        self.body_bytes().fill_(byte)


def window(shape, dtype, device, margin_fill, body=None, row_bytes=None, what="window"):
    """One uint8 allocation holding [margin | body | margin]; returns the Window whose `.view` has `shape` / `dtype`.
    margin_fill: a byte (POISON, GUARD) or INT_POISON.  body: None = the margin's fill, a byte, or a tensor copied in (same shape; any
    dtype of the same element size is taken by its bits).  row_bytes: the widest row a kernel addresses the buffer by, when that is not
    the last dimension (a flat workspace carved into rows)."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    item = _itemsize(dtype)
    numel = 1
    for s in shape:
        numel *= s
    nbytes = numel * item
    if row_bytes is None:
        row_bytes = (shape[-1] if len(shape) >= 2 else 1) * item
    margin = max(MIN_MARGIN, TILE_ROWS * row_bytes)
    margin = (margin + ALIGN - 1) // ALIGN * ALIGN
    tail_pad = (-nbytes) % 4                      # the back margin starts on a 4-byte boundary (INT_POISON pattern phase)
    total = margin + ALIGN + nbytes + tail_pad + margin
    base = torch.empty(total, dtype=torch.uint8, device=device)
    assert base.data_ptr() % 4 == 0
    assert margin_fill != INT_POISON or (item == 4 and not tail_pad), "INT_POISON margins are for int32 windows"
    base.copy_(_pattern(margin_fill, total, base.device))
    start = margin + (-(base.data_ptr() + margin)) % ALIGN
    view = base[start:start + nbytes].view(dtype).view(shape)
    assert view.data_ptr() % ALIGN == 0 and view.data_ptr() == base.data_ptr() + start
    w = Window(base, view, start, nbytes, margin, margin_fill, what)
    if body is None:
        pass
    elif isinstance(body, int):
        w.refill_body(body)
    else:
        src = body.to(device).contiguous()
        assert tuple(src.shape) == shape or src.numel() * src.element_size() == nbytes, (tuple(src.shape), shape)
        w.body_bytes().copy_(src.view(torch.uint8).reshape(-1))
    return w


def poison_pad_rows(t, valid_rows, byte=POISON):
    """Rows valid_rows .. of a ceil256-row operand (contiguous, rows first) filled with 0xff: NaN in every float format."""
    assert t.is_contiguous() and 0 <= valid_rows <= t.shape[0]
    if valid_rows < t.shape[0]:
        t[valid_rows:].view(torch.uint8).fill_(byte)
    return t


def bits(t):
    """The tensor's bytes (contiguous copy if needed) for bit-for-bit comparisons."""
    return t.contiguous().view(torch.uint8).reshape(-1)


def same_bits(a, b):
    """Bit-for-bit equality of two tensors of equal byte size; on failure the first differing byte offset."""
    ba, bb = bits(a).cpu(), bits(b).cpu()
    assert ba.numel() == bb.numel(), (ba.numel(), bb.numel())
    bad = (ba != bb).nonzero()
    assert bad.numel() == 0, f"bits differ: first at byte {int(bad[0])} of {ba.numel()}, {bad.numel()} bytes in all"
    return True


def all_bytes(t, byte):
    """Every byte of t equals `byte`; on failure the first offset that does not."""
    b = bits(t)
    bad = (b != byte).nonzero()
    assert bad.numel() == 0, f"byte at offset {int(bad[0])} of {b.numel()} is 0x{int(b[int(bad[0])]):02x}, not 0x{byte:02x} ({bad.numel()} bytes changed)"
    return True


# ------------------------------------------------------------------------------------------------ one call, twice
# The three assertions of every footprint test (DESIGN.md "Memory contracts"), for a call described by its argument list:
#   A1  the contract call's outputs equal the plain call's, bit for bit;
#   A2  every margin of every argument is intact (read-only arguments too);
#   A3  bytes of an output the header says are not written keep GUARD.
# Plain call: tight, separately allocated tensors, input pad rows as given (zero), workspaces roomy and zero-filled.
# Contract call: every argument a window -- inputs in POISON margins with POISON pad rows, int inputs in INT_POISON margins, outputs
# in GUARD margins with a GUARD body, workspaces of exactly the stated size, POISON-filled, in GUARD margins.
class In:
    """Read-only tensor argument.  valid_rows: rows from there on are pad rows (zero in the plain call, POISON in the contract call)."""

    def __init__(self, t, valid_rows=None, fill=POISON, row_bytes=None):
        self.t, self.valid_rows, self.fill, self.row_bytes = t, valid_rows, fill, row_bytes


class IntIn(In):
    """int32 input whose stray values must be loud: INT_POISON margins."""

    def __init__(self, t):
        super().__init__(t.to(torch.int32), None, INT_POISON)


class Out:
    """Output.  written(view) -> the part A1 compares (default: all of it; a list of tensors is fine); keep(view) -> the part(s) that
    must still hold GUARD afterwards (A3).  init: a tensor for read-modify-write outputs (both calls start from it), else GUARD."""

    def __init__(self, shape, dtype, written=None, keep=None, init=None, row_bytes=None):
        self.shape, self.dtype, self.written, self.keep, self.init, self.row_bytes = tuple(shape), dtype, written, keep, init, row_bytes


class Work:
    """Workspace of exactly `nbytes` in the contract call (POISON body, GUARD margins); plain: max(plain_bytes, nbytes) zero bytes."""

    def __init__(self, nbytes, plain_bytes=0, row_bytes=None):
        self.nbytes, self.plain_bytes, self.row_bytes = int(nbytes), int(plain_bytes), row_bytes


class SizeOf:
    """Scalar argument: the byte size of the workspace at position `index` as each call has it (roomy / exact)."""

    def __init__(self, index):
        self.index = index


def _parts(sel, view):
    if sel is None:
        return [view]
    got = sel(view)
    return list(got) if isinstance(got, (list, tuple)) else [got]


class Calls:
    """Both calls' arguments: plain[i] (tensor) and win[i] (Window) per argument, None for scalars."""

    def __init__(self, specs, device):
        self.specs, self.device = list(specs), device
        self.plain, self.win = [], []
        for i, s in enumerate(self.specs):
            what = f"argument {i} ({type(s).__name__})"
            if isinstance(s, In):
                src = s.t.contiguous()
                p = src.to(device).clone()
                w = window(src.shape, src.dtype, device, s.fill, body=src, row_bytes=s.row_bytes, what=what)
                if s.valid_rows is not None:
                    poison_pad_rows(w.view, s.valid_rows)
            elif isinstance(s, Out):
                p = torch.empty(s.shape, dtype=s.dtype, device=device)
                p.view(torch.uint8).fill_(GUARD)
                if s.init is not None:
                    p.copy_(s.init.to(device))
                w = window(s.shape, s.dtype, device, GUARD, body=s.init, row_bytes=s.row_bytes, what=what)
            elif isinstance(s, Work):
                p = torch.zeros(max(s.nbytes, s.plain_bytes, 256), dtype=torch.uint8, device=device)
                w = window((max(s.nbytes, 1),), torch.uint8, device, GUARD, body=POISON, row_bytes=s.row_bytes, what=what)
            else:
                p = w = None
            self.plain.append(p)
            self.win.append(w)

    def args(self, contract, as_arg):
        out = []
        for s, p, w in zip(self.specs, self.plain, self.win):
            if isinstance(s, SizeOf):
                out.append(self.win[s.index].nbytes if contract else self.plain[s.index].numel())
            elif p is None:
                out.append(s)
            else:
                out.append(as_arg(w.view if contract else p))
        return out

    def check(self, what=""):
        for i, (s, p, w) in enumerate(zip(self.specs, self.plain, self.win)):
            if w is None:
                continue
            tag = f"{what} argument {i}"
            off = w.margin_damage()                                                  # A2
            assert off is None, f"{tag}: margin byte at offset {off} of a {w.nbytes}-byte window changed"
            if isinstance(s, In):                                                    # read-only: the bits it was given
                ref = p.clone()
                if s.valid_rows is not None:
                    poison_pad_rows(ref, s.valid_rows)
                assert same_bits(w.view, ref), tag
                assert same_bits(p, s.t), tag
            elif isinstance(s, Out):
                if s.init is None:                                                   # (the call did store its result: not a no-op)
                    assert any(bool((bits(a) != GUARD).any()) for a in _parts(s.written, w.view)), f"{tag}: nothing was written"
                for a, b in zip(_parts(s.written, w.view), _parts(s.written, p)):    # A1
                    try:
                        same_bits(a, b)
                    except AssertionError as e:
                        raise AssertionError(f"{tag}: contract call != plain call: {e}") from None
                if s.keep is not None:                                               # A3: GUARD, or the bytes it started from
                    want = None if s.init is None else _parts(s.keep, s.init.to(w.view.device))
                    for j, a in enumerate(_parts(s.keep, w.view)):
                        try:
                            all_bytes(a, GUARD) if want is None else same_bits(a, want[j])
                        except AssertionError as e:
                            raise AssertionError(f"{tag}: bytes the contract leaves alone were written: {e}") from None
        return True


def run_both(fn, specs, device, as_arg=None, what=""):
    """fn(*args) is called twice -- plain, then contract -- with tensor arguments converted by as_arg (default: ctypes void pointers);
    then A1 / A2 / A3.  Returns the Calls (plain tensors and windows) for further assertions."""
    if as_arg is None:
        import ctypes
        as_arg = lambda t: ctypes.c_void_p(t.data_ptr())         # noqa: E731
    calls = Calls(specs, device)
    fn(*calls.args(False, as_arg))
    fn(*calls.args(True, as_arg))
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    calls.check(what)
    return calls
