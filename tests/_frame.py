"""A guarded device buffer for tests of what an entry point writes: exactly its output, from any element-aligned pointer.

Frame(count, lead, back_extra) is one device allocation of FRONT + lead + count + BACK + back_extra elements, every one
holding SENTINEL_BITS (a NaN no evaluation produces; doubles: two such words).  The payload -- the `count` elements the
call under test owns -- starts FRONT + lead elements in.  The allocation's base is 256-byte aligned (asserted), so a
float payload of lead k sits at 4 k mod 16 bytes.  result() copies the buffer back and checks, by bits, that every guard
element still holds the sentinel and that no payload element does (with `written=`: exactly the masked ones do not).

check_words is that check on a host array: it needs no GPU and has CPU tests (tests/test_gpu_output_frame.py).
"""
import ctypes as C

import numpy as np

SENTINEL_BITS = 0x7fa5a5a5
SENTINEL_BITS64 = (SENTINEL_BITS << 32) | SENTINEL_BITS
FRONT = BACK = 4096


def sentinel_of(words):
    return np.uint64(SENTINEL_BITS64) if words.dtype == np.uint64 else np.uint32(SENTINEL_BITS)


def check_words(words, start, count, written=None, what="frame"):
    """`words`: the whole buffer as unsigned integers (uint32 for float, uint64 for double); the payload is
    words[start:start + count].  Raises AssertionError naming the first offending element, as an offset relative to the
    payload (negative in front of it, >= count behind it):
      * a guard element that no longer holds the sentinel;
      * a payload element that still holds it (written=None), or, with a boolean mask `written` of `count` elements, a
        masked element that still holds it or an unmasked one that does not (it must be left untouched)."""
    words = np.asarray(words)
    assert words.dtype in (np.uint32, np.uint64) and words.ndim == 1, words.dtype
    assert 0 <= start and start + count <= words.size, (start, count, words.size)
    is_sentinel = words == sentinel_of(words)
    front = np.flatnonzero(~is_sentinel[:start])
    assert front.size == 0, \
        f"{what}: {front.size} elements in front of the output were written, first at offset {int(front[0]) - start}"
    back = np.flatnonzero(~is_sentinel[start + count:])
    assert back.size == 0, \
        f"{what}: {back.size} elements behind the output were written, first at offset {int(back[0]) + count}"
    payload = is_sentinel[start:start + count]
    if written is None:
        left = np.flatnonzero(payload)
        assert left.size == 0, f"{what}: {left.size} of {count} output elements were not written, first at index {int(left[0])}"
        return
    written = np.asarray(written).astype(bool).reshape(-1)
    assert written.size == count, (written.size, count)
    left = np.flatnonzero(payload & written)
    assert left.size == 0, f"{what}: {left.size} active output elements were not written, first at index {int(left[0])}"
    touched = np.flatnonzero(~payload & ~written)
    assert touched.size == 0, \
        f"{what}: {touched.size} inactive output elements were written, first at index {int(touched[0])}"


class Frame:
    """The device buffer.  dtype: np.float32 or np.float64.  `ptr`: the payload as a ctypes pointer for the C ABI; `tensor`:
    the payload as a flat torch view (for helpers that take an `out=` tensor, and for comparisons on the device)."""

    def __init__(self, count, lead, back_extra=0, dtype=np.float32):
        import torch
        self.dtype = np.dtype(dtype)
        assert self.dtype in (np.dtype(np.float32), np.dtype(np.float64)), dtype
        assert count >= 0 and lead >= 0 and back_extra >= 0
        self.count, self.lead, self.start = int(count), int(lead), FRONT + int(lead)
        total = self.start + self.count + BACK + int(back_extra)
        wide = self.dtype.itemsize == 8
        self.buf = torch.empty(total, dtype=torch.float64 if wide else torch.float32, device="cuda")
        assert self.buf.data_ptr() % 256 == 0, hex(self.buf.data_ptr())
        if wide:
            self.buf.view(torch.int64).fill_(int(np.uint64(SENTINEL_BITS64).view(np.int64)))
        else:
            self.buf.view(torch.int32).fill_(int(np.uint32(SENTINEL_BITS).view(np.int32)))
        self.tensor = self.buf[self.start:self.start + self.count]
        self.ptr = C.c_void_p(self.buf.data_ptr() + self.start * self.dtype.itemsize)
        assert self.ptr.value % 16 == (self.lead * self.dtype.itemsize) % 16

    @classmethod
    def holding(cls, array, lead):
        """A frame whose payload holds `array` (an input list for the call under test)."""
        import torch
        a = np.ascontiguousarray(array)
        f = cls(a.size, lead, dtype=a.dtype)
        f.tensor.copy_(torch.from_numpy(a.reshape(-1)))
        return f

    def result(self, written=None, what="frame"):
        """Synchronises, checks the guards and the payload (check_words) and returns the payload as a host array."""
        import torch
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        check_words(host.view(np.uint64 if self.dtype.itemsize == 8 else np.uint32), self.start, self.count, written,
                    f"{what}, lead {self.lead}")
        return host[self.start:self.start + self.count]
