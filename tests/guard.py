"""A matrix in a guard: `rows` rows of `row_len` 32-bit words, `ld` words apart, between a front and a back guard.

What a launch is allowed to touch is the [rows, row_len] payload. Everything else in the allocation -- the `ld - row_len` words
between the rows, FRONT words in front of row 0, and behind the last row the whole tile the kernels may have rounded the matrix up
to, (roundup(rows, 128) - rows) * ld + 128 words -- holds one fill pattern and is compared word for word (uint32) afterwards:

  outputs  NAN_BITS, one fixed quiet-NaN pattern: a stray store of ANY value shows, and a kernel that reads its output's gap as an
           operand (dst aliasing add2) poisons its result;
  inputs   GAP_IN = 1e30: fmaxf drops a NaN, so a NaN in a gap would hide from the quantizers' amax -- a stray 1e30 changes it.

With ld == row_len a store to "row M + j of column n" of a column-major [n][m] result lands on the payload of column n + 1, where its
rightful owner may overwrite it in the same launch; only ld > row_len gives such a store a gap to land in. Host-only module: the
device copy goes through whatever `upload` / `download` the caller hands in (tests/test_guard_cpu.py runs it on numpy alone).
"""
import numpy as np

NAN_BITS = np.uint32(0x7FC5A5A5)                                   # a quiet NaN no arithmetic of the kernels produces
GAP_IN = np.float32(1e30)
GAP_IN_BITS = np.array([GAP_IN], np.float32).view(np.uint32)[0]
FRONT = 128                                                        # words in front of row 0
TILE = 128                                                         # the widest tile a kernel rounds the matrix up to


class GuardError(AssertionError):
    pass


class Guard:
    def __init__(self, rows, row_len, ld=None, fill=NAN_BITS, payload=None, dtype=np.float32):
        ld = row_len if ld is None else int(ld)
        assert rows >= 1 and row_len >= 1 and ld >= row_len and np.dtype(dtype).itemsize == 4
        self.rows, self.row_len, self.ld, self.dtype = int(rows), int(row_len), ld, np.dtype(dtype)
        self.fill = np.uint32(fill)
        self.back = ((rows + TILE - 1) // TILE * TILE - rows) * ld + 128
        self.words = FRONT + rows * ld + self.back
        self.offset = FRONT                                        # word index of payload element (0, 0)
        self._payload = None if payload is None else np.ascontiguousarray(payload, self.dtype).reshape(rows, row_len)
        self.buf = None                                            # the device allocation, when there is one

    # ---- host side
    def _body(self, image):
        return image[FRONT:FRONT + self.rows * self.ld].reshape(self.rows, self.ld)

    def image(self):
        """the allocation's initial contents (uint32): fill everywhere, the payload (when given) in its place"""
        im = np.full(self.words, self.fill, np.uint32)
        if self._payload is not None:
            self._body(im)[:, :self.row_len] = self._payload.view(np.uint32)
        return im

    def check(self, image=None):
        """the [rows, row_len] payload of `image` (default: the device copy); GuardError naming the first (row, column) -- counted
        from payload element (0, 0) at stride ld, so row -1 is the front guard and row >= rows the back guard -- when a guard or
        gap word no longer holds the fill pattern"""
        if image is None:
            image = self.download()
        image = np.ascontiguousarray(image).view(np.uint32).ravel()
        assert image.size == self.words, (image.size, self.words)
        outside = np.ones(self.words, bool)
        self._body(outside)[:, :self.row_len] = False
        bad = np.flatnonzero(outside & (image != self.fill))
        if bad.size:
            rel = int(bad[0]) - FRONT
            raise GuardError("%d word(s) outside the %d x %d payload (stride %d) changed; the first is (row %d, column %d) = 0x%08X"
                             % (bad.size, self.rows, self.row_len, self.ld, rel // self.ld, rel % self.ld, int(image[bad[0]])))
        return self._body(image)[:, :self.row_len].copy().view(self.dtype)

    # ---- device side (ggllm_cpp_amd.DevBuf)
    def to_device(self):
        import ggllm_cpp_amd as g
        self.buf = g.DevBuf(host=self.image())
        return self

    @property
    def ptr(self):
        """device address of payload element (0, 0)"""
        return self.buf.ptr + 4 * FRONT

    def download(self):
        return self.buf.to_host(np.uint32, (self.words,))

    def free(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None


def out_guard(rows, row_len, ld=None, payload=None):
    """an output matrix on the device: NaN pattern in guards and gaps (and in the payload, unless one is given: dst aliasing an input)"""
    return Guard(rows, row_len, ld, NAN_BITS, payload).to_device()


def in_guard(payload, ld=None):
    """an input matrix [rows, row_len] on the device with 1e30 in guards and gaps"""
    payload = np.ascontiguousarray(payload, np.float32)
    payload = payload.reshape(-1, payload.shape[-1])
    return Guard(payload.shape[0], payload.shape[1], ld, GAP_IN_BITS, payload).to_device()
