"""Guard-band frames for kernel tests: a logical tensor as a strided view inside ONE flat allocation whose every other element holds a sentinel.

An OUTPUT frame is filled with a NaN-payload sentinel (bf16 0x7FC1, fp32 0x7FC00001, fp16 0x7E01, bytes 0x5A); after the launch
  assert_untouched()    every element outside the view still has the sentinel's bits (compared as integers: a NaN written over a NaN of another payload counts)
  assert_all_written()  no sentinel is left inside the view (for floats only a NaN of exactly that payload counts; 0x5A is also a legitimate e4m3 byte, so for byte
                        outputs a caller compares with a dense run's bits instead)
An INPUT frame (Frame.of(data, ...)) holds the data in the view and a poison around it (NaN by default, or a caller-given value); the caller may write
other poison into .padded / .buf before seal() takes the snapshot that assert_unchanged() compares the WHOLE buffer with.

Layout of the flat buffer, in elements:  [front guard | batch 0: rows x ld | gap | batch 1 ... | tail guard of tail_rows x ld]
  element (b, r, c) of the view sits at  front + b * batch_stride + r * ld + c.  Columns [cols, ld) are row padding, rows behind `rows` of a slice the
  inter-batch gap (batch_stride > rows * ld), everything behind the last slice's last row the tail guard.
Sizing is a SAFETY rule, not a convenience: a kernel that stored a whole unmasked workgroup tile must still land inside the frame's own allocation and be caught
by comparison, never by a fault -- frame_for_tile() sizes the tail and the row stride from the tile, and nothing here relies on a fault.

Positions in a failure report are (batch, row, col) relative to the view's origin: col >= cols is row padding, row >= rows the gap behind that slice (the tail guard
behind the last one); the front guard is reported as batch -1 with col counted backwards from the origin (-1 = the element directly in front of it).
"""
import math

import torch

_INT = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8, torch.int32: torch.int32,
        torch.int8: torch.int8, torch.int64: torch.int64}
# raw bits, as the signed integer of the same width holds them
SENTINEL = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01, torch.float32: 0x7FC00001, torch.uint8: 0x5A, torch.int8: 0x5A, torch.int32: 0x5A5A5A5A,
            torch.int64: 0x5A5A5A5A5A5A5A5A}
ALT_NAN = {torch.bfloat16: 0x7FC2, torch.float16: 0x7E02, torch.float32: 0x7FC00002}      # a NaN with another payload (the detector's own test writes it)


class FrameError(AssertionError):
    """a frame check failed: .count elements differ, .positions holds the first few as (batch, row, col)"""

    def __init__(self, msg, count, positions):
        super().__init__(msg)
        self.count, self.positions = count, positions


def round_up(n, m):
    return (n + m - 1) // m * m


class Frame:
    def __init__(self, shape, dtype, ld=None, batch_stride=None, front=64, tail_rows=256, fill=None, device="cpu", name="frame", storage=None):
        """shape: the logical tensor; its last axis is the column axis, the one before it the row axis, everything in front of those the batch (flattened;
        more than one batch axis only with the dense batch stride).  ld: row stride (default: dense), batch_stride: elements between slices (default: rows * ld),
        front: guard elements in front of the view, tail_rows: guard rows of ld elements behind it.  fill: the sentinel's raw bits (default: SENTINEL[dtype]).
        storage: a flat tensor of exactly .numel elements of dtype to live in (two frames that an ABI addresses relative to each other share one allocation)."""
        shape = tuple(int(s) for s in shape)
        assert len(shape) >= 1 and all(s > 0 for s in shape) and dtype in _INT
        self.shape, self.dtype, self.name = shape, dtype, name
        self.cols = shape[-1]
        self.rows = shape[-2] if len(shape) >= 2 else 1
        self.batch = math.prod(shape[:-2]) if len(shape) > 2 else 1
        self.ld = self.cols if ld is None else int(ld)
        self.batch_stride = self.rows * self.ld if batch_stride is None else int(batch_stride)
        assert self.ld >= self.cols and self.batch_stride >= self.rows * self.ld and front >= 0 and tail_rows >= 0
        self.front, self.tail_rows = int(front), int(tail_rows)
        self.sentinel = SENTINEL[dtype] if fill is None else int(fill)
        self.span = (self.batch - 1) * self.batch_stride + (self.rows - 1) * self.ld + self.cols       # first element behind the view's last one
        self.numel = self.front + (self.batch - 1) * self.batch_stride + self.rows * self.ld + self.tail_rows * self.ld
        if storage is None:
            self.bits = torch.full((self.numel,), _wrap(self.sentinel, _INT[dtype]), dtype=_INT[dtype], device=device)
        else:
            assert storage.dim() == 1 and storage.numel() == self.numel and storage.dtype == dtype and storage.is_contiguous()
            self.bits = storage.view(_INT[dtype])
            self.bits.fill_(_wrap(self.sentinel, _INT[dtype]))
            device = storage.device
        self.buf = self.bits.view(dtype)                                                   # the flat allocation as the kernel's type
        self.origin = self.buf.storage_offset() + self.front                               # as_strided counts from the storage, not from the slice
        v3 = self.buf.as_strided((self.batch, self.rows, self.cols), (self.batch_stride, self.ld, 1), self.origin)
        if len(shape) == 3:
            self.view = v3
        elif len(shape) == 2:
            self.view = v3[0]
        elif len(shape) == 1:
            self.view = v3[0, 0]
        else:
            assert self.batch_stride == self.rows * self.ld, "several batch axes need the dense batch stride"
            self.view = self.buf.as_strided(shape, _strides(shape, self.ld), self.origin)
        self._view_bits = self.bits.as_strided((self.batch, self.rows, self.cols), (self.batch_stride, self.ld, 1), self.origin)
        inside = torch.zeros(self.numel, dtype=torch.bool, device=device)
        inside.as_strided((self.batch, self.rows, self.cols), (self.batch_stride, self.ld, 1), self.front).fill_(True)
        self.inside = inside
        self._snapshot = None

    # ------------------------------------------------------------------ construction helpers
    @classmethod
    def of(cls, data, ld=None, batch_stride=None, front=64, tail_rows=8, poison=None, name="input"):
        """INPUT frame around `data` (any strides; copied): poison = None -> the dtype's NaN sentinel (0x5A.. for integer types), a float / int -> that value."""
        f = cls(data.shape, data.dtype, ld=ld, batch_stride=batch_stride, front=front, tail_rows=tail_rows, device=data.device, name=name)
        if poison is not None:
            f.buf.fill_(poison)
        f.view.copy_(data)
        return f

    @property
    def padded(self):
        """[batch, rows, ld]: the view's rows with their padding columns (the last row's padding lies in the gap / tail guard)"""
        return self.buf.as_strided((self.batch, self.rows, self.ld), (self.batch_stride, self.ld, 1), self.origin)

    def rows_behind(self, n):
        """[batch, n, ld]: the n rows behind the last logical row of every slice (gap rows; for the last slice the head of the tail guard)"""
        assert n <= self.tail_rows and (self.batch == 1 or n * self.ld <= self.batch_stride - self.rows * self.ld)
        return self.buf.as_strided((self.batch, n, self.ld), (self.batch_stride, self.ld, 1), self.origin + self.rows * self.ld)

    def seal(self):
        self._snapshot = self.bits.clone()
        return self

    def data_ptr(self):
        return self.view.data_ptr()

    # ------------------------------------------------------------------ checks
    def position(self, offset):
        """(batch, row, col) of a flat buffer offset, relative to the view's origin"""
        o = int(offset) - self.front
        if o < 0:
            return (-1, 0, o)
        b = min(o // self.batch_stride, self.batch - 1)
        o -= b * self.batch_stride
        return (b, o // self.ld, o % self.ld)

    def _fail(self, what, bad_flat):
        idx = torch.nonzero(bad_flat.reshape(-1), as_tuple=False).reshape(-1)
        pos = [self.position(i) for i in idx[:8].tolist()]
        raise FrameError(f"{self.name}: {what}: {idx.numel()} element(s), first at (batch, row, col) = {pos}", int(idx.numel()), pos)

    def assert_untouched(self):
        bad = (self.bits != _wrap(self.sentinel, self.bits.dtype)) & ~self.inside
        if bool(bad.any()):
            self._fail("elements outside the logical view were written", bad)

    def assert_all_written(self):
        bad = (self.bits == _wrap(self.sentinel, self.bits.dtype)) & self.inside
        if bool(bad.any()):
            self._fail("elements of the logical view still hold the sentinel", bad)

    def assert_unchanged(self):
        assert self._snapshot is not None, "seal() the input frame before the launch"
        bad = self.bits != self._snapshot
        if bool(bad.any()):
            self._fail("an input buffer was written", bad)

    def touched_positions(self):
        """every changed guard element as (batch, row, col) (for tests of the detector itself)"""
        bad = (self.bits != _wrap(self.sentinel, self.bits.dtype)) & ~self.inside
        return [self.position(i) for i in torch.nonzero(bad, as_tuple=False).reshape(-1).tolist()]


def _wrap(bits, int_dtype):
    """the Python int whose two's-complement pattern in int_dtype is `bits`"""
    if int_dtype == torch.uint8:
        return bits & 0xFF
    n = torch.iinfo(int_dtype).bits
    bits &= (1 << n) - 1
    return bits - (1 << n) if bits >= 1 << (n - 1) else bits


def _strides(shape, ld):
    st = [1] * len(shape)
    st[-2] = ld
    for i in range(len(shape) - 3, -1, -1):
        st[i] = st[i + 1] * shape[i + 1]
    return tuple(st)


def out_ld(width, tile_cols, align=8):
    """row stride of a ragged-N output: at least the width rounded up to the tile width, plus 8 (so a full unmasked tile row stays inside its own row), kept a
    multiple of `align` elements (8 bf16 = 16 bytes; 16 for e4m3 bytes)"""
    return round_up(round_up(width, max(1, tile_cols)) + 8, align)


def frame_for_tile(shape, dtype, tile_rows=256, tile_cols=0, extra_batch_rows=3, front=64, align=8, device="cpu", name="out", ld=None, batch_stride=None):
    """OUTPUT frame sized by the safety rule for a kernel whose workgroup tile is tile_rows x tile_cols: ld by out_ld (tile_cols = 0: width + 8), a batch stride of
    extra_batch_rows rows more than the slice, a tail guard of one full tile of rows (never fewer than 256 where no tile is known)."""
    shape = tuple(shape)
    cols, rows = shape[-1], (shape[-2] if len(shape) >= 2 else 1)
    if ld is None:
        ld = out_ld(cols, tile_cols, align) if tile_cols else round_up(cols + 8, align)
    if batch_stride is None:
        batch_stride = (rows + extra_batch_rows) * ld
    return Frame(shape, dtype, ld=ld, batch_stride=batch_stride, front=front, tail_rows=max(int(tile_rows), 1) + extra_batch_rows, device=device, name=name)


def dense_guarded(shape, dtype, rows=256, front=64, device="cpu", name="out"):
    """OUTPUT frame for an entry that is dense by contract: the view is contiguous, the guards sit in front of and behind it only"""
    shape = tuple(shape)
    return Frame(shape, dtype, front=front, tail_rows=rows, device=device, name=name)
