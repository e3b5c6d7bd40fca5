"""Guard bands for tests that call libgoalnet_hip.so through the raw C ABI (cvml_goalnet_amd._lib), not through ops.py.

ops.py allocates every output with torch.empty(exact size) and every workspace from the library's own *_ws_bytes, and the
caching allocator rounds each block up: a store one row or 16 bytes past an output lands in slack that nobody reads. Here
every buffer a kernel may write is a VIEW in the middle of one larger tensor that the test owns:

    [ band >= 1 MiB | payload (start 16-byte aligned) | band >= 1 MiB ]

The bands hold a fixed bit pattern (quiet NaN of the payload's float type; 0xA5 bytes for integer types) and are compared bit
for bit afterwards. Both bands are part of the test's own allocation, so an overrun is observed, never faulted on. A failing
band check is a finding about the kernel: report it and fix the kernel; never wrap it in a retry.

Inputs go through `place()`: the same layout with NaN bands around a copy of the tensor, and the usual parity check is made on
the outputs. This catches only over-reads that PROPAGATE: a value read beyond the input that reaches an output turns it to NaN
(or, for an integer input, to a wildly wrong value); an over-read whose value is discarded, masked or multiplied away in
integer arithmetic is not seen. For the zero-padded 16-bit layouts of goalnet_bf16_padded_layout the guard pixels inside
total_elems are zero by contract; the whole total_elems buffer is the payload and the NaN bands lie outside it.
"""
from __future__ import annotations

import torch

BAND_BYTES = 1 << 20
ALIGN = 16

# quiet-NaN bit patterns, as an integer type of the same width
_NAN_BITS = {
    torch.float32: (torch.int32, 0x7FC00000),
    torch.float64: (torch.int64, 0x7FF8000000000000),
    torch.bfloat16: (torch.int16, 0x7FC0),
    torch.float16: (torch.int16, 0x7E00),
}
_INT_BYTE = 0xA5


def ptr(t):
    """device address of a tensor for a ctypes c_void_p argument (None -> NULL)"""
    return 0 if t is None else t.data_ptr()


class Bands:
    """All guarded buffers of one test. `guarded` / `place` hand out views; `assert_bands_intact` checks every band."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._items = []     # (name, raw uint8 buffer, pristine copy, [(byte offset, byte length) of payload runs])

    def _alloc(self, name, nbytes, dtype, runs_of):
        item = torch.empty((), dtype=dtype).element_size()
        span = -(-nbytes // ALIGN) * ALIGN
        raw = torch.empty(BAND_BYTES + span + BAND_BYTES, dtype=torch.uint8, device=self.device)
        assert raw.data_ptr() % ALIGN == 0 and BAND_BYTES % ALIGN == 0 and BAND_BYTES % item == 0
        if dtype in _NAN_BITS:
            ity, bits = _NAN_BITS[dtype]
            raw.view(ity).fill_(bits)
        else:
            raw.fill_(_INT_BYTE)
        pristine = raw.clone()
        payload = raw[BAND_BYTES:BAND_BYTES + nbytes].view(dtype)
        assert payload.data_ptr() % ALIGN == 0
        self._items.append((name, raw, pristine, runs_of(BAND_BYTES, item)))
        return payload

    def guarded(self, shape, dtype, fill=None, name=None):
        """A contiguous view of `shape` between two bands. fill=None leaves the payload holding the band pattern (an output
        element that the kernel never writes then shows up as NaN / 0xA5 in the parity check); a number fills it; a tensor is
        copied in."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = 1
        for s in shape:
            n *= int(s)
        item = torch.empty((), dtype=dtype).element_size()
        view = self._alloc(name or f"buf{len(self._items)}", n * item, dtype, lambda off, it: [(off, n * it)]).view(shape)
        if fill is not None:
            if torch.is_tensor(fill):
                view.copy_(fill.to(device=self.device, dtype=dtype).reshape(shape))
            else:
                view.fill_(fill)
        return view

    def guarded_rows(self, rows, cols, ld, dtype, fill=None, name=None):
        """A (rows, cols) view with row stride `ld` >= cols elements; the ld - cols elements between the rows are bands too
        (the last row has no gap behind it: the buffer ends with its last column)."""
        assert ld >= cols and rows >= 1
        n = (rows - 1) * ld + cols
        flat = self._alloc(name or f"buf{len(self._items)}", n * torch.empty((), dtype=dtype).element_size(), dtype,
                           lambda off, it: [(off + r * ld * it, cols * it) for r in range(rows)])
        view = flat.as_strided((rows, cols), (ld, 1))
        if fill is not None:
            if torch.is_tensor(fill):
                view.copy_(fill.to(device=self.device, dtype=dtype).reshape(rows, cols))
            else:
                view.fill_(fill)
        return view

    def place(self, t, name=None):
        """An input: a copy of `t` (contiguous) between NaN / 0xA5 bands. See the module docstring for what this can show."""
        return self.guarded(tuple(t.shape), t.dtype, fill=t, name=name or f"in{len(self._items)}")

    def place_rows(self, t, ld, name=None):
        """A 2-D input with row stride ld, the gaps between rows holding the band pattern"""
        return self.guarded_rows(t.shape[0], t.shape[1], ld, t.dtype, fill=t, name=name or f"in{len(self._items)}")

    def assert_bands_intact(self):
        torch.cuda.synchronize(self.device)
        for name, raw, pristine, runs in self._items:
            cur = raw.clone()
            for off, ln in runs:                       # blank the payload; everything else must be the pattern, bit for bit
                cur[off:off + ln] = pristine[off:off + ln]
            if not torch.equal(cur, pristine):
                bad = (cur != pristine).nonzero().flatten()
                first, last = int(bad[0]), int(bad[-1])
                lo, hi = runs[0][0], runs[-1][0] + runs[-1][1]
                where = "before the payload" if last < lo else "behind the payload" if first >= hi else "in or around the payload rows"
                raise AssertionError(f"guard band of '{name}' overwritten: {bad.numel()} bytes differ, {where}; first at payload "
                                     f"offset {first - lo}, last at {last - lo} (payload spans {hi - lo} bytes)")


def bits_equal(a, b):
    """bit-for-bit equality of two tensors of the same dtype and shape (NaN payloads and signed zeros included)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    ity = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(ity), b.contiguous().view(ity))
