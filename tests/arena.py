"""A guarded arena for calling the C ABI directly: every operand of a call lives inside ONE flat buffer, apart from its
neighbours by guard bands, so that a kernel that writes past an output or a workspace, reads what it never wrote, ignores a batch
stride or leaves part of an output unwritten is caught - and an overrun of up to a guard band lands inside the allocation, never
outside the process's memory.

    a = Arena("cuda")
    x = a.place_input(x_host, bstride=(Cin + 8) * H * W)      # samples `bstride` floats apart, NaN in between
    ws = a.place_ws(n)                                         # exactly n floats, NaN-prefilled
    dw = a.place_output((Cout, Cin, 3, 3))
    dx = a.place_inout(base, bstride=(Cin + 2) * H * W + 1)   # what an accumulating call adds to: read and written, gaps guarded
    rc = L.tgsr_...(x.ptr, ..., ws.ptr, dw.ptr, ...)           # the first .ptr allocates the buffer
    a.check()
    got = dw.read()

The buffer is int32 words; PATTERN is a quiet NaN no arithmetic produces (the payload of a NaN an operation makes is the canonical
0x7FC00000 or an operand's), so "this word was never written" is a bit comparison.  Guard bands, the gaps between the samples of a
strided operand and every input hold PATTERN / their values before the call and must hold the same bits after it; the interior of
an output must hold no PATTERN word and only finite values; a workspace may be left partly unwritten but not overrun.  A uint8
input (a mask) is padded to whole words, the padding bytes holding PATTERN's.
"""
import ctypes

import numpy as np
import torch

PATTERN = 0x7FC5A5A5
GUARD = 16384             # words on each side of every operand: more than two image rows plus a tile at every shape of the suite

_INPUT, _OUTPUT, _WS, _INOUT, _ABSENT = "input", "output", "ws", "inout", "absent"


class Region:
    """One operand: `nb` samples of `per` words, `bstride` words apart, the first at word `offset` of the arena."""

    def __init__(self, arena, kind, offset, shape, nb, per, bstride, dtype, host):
        self.arena, self.kind, self.offset, self.shape = arena, kind, offset, tuple(shape)
        self.nb, self.per, self.bstride, self.dtype, self.host = nb, per, bstride, dtype, host

    @property
    def span(self):
        return (self.nb - 1) * self.bstride + self.per

    @property
    def address(self):
        return self.arena.base_address() + 4 * self.offset

    @property
    def ptr(self):
        return ctypes.c_void_p(self.address)

    def slices(self):
        """(first word, one past the last) of every run of interior words: one per sample, or one in all where they are dense."""
        if self.bstride == self.per or self.nb == 1:
            return [(self.offset, self.offset + self.nb * self.per)]
        return [(self.offset + b * self.bstride, self.offset + b * self.bstride + self.per) for b in range(self.nb)]

    def words(self):
        """The interior as int32 words on the host, [nb * per]."""
        buf = self.arena.buffer()
        return torch.cat([buf[lo:hi] for lo, hi in self.slices()]).cpu()

    def read(self):
        """The interior as a host tensor of the operand's shape and type."""
        if self.dtype == torch.uint8:          # a byte operand: whole words, the padding bytes behind the last element dropped
            return self.words().view(torch.uint8)[:int(np.prod(self.shape))].reshape(self.shape).clone()
        return self.words().view(self.dtype).reshape(self.shape).clone()


class Arena:
    def __init__(self, device, guard=GUARD):
        assert guard >= 1
        self.device, self.guard = torch.device(device), guard
        self.regions, self._cursor, self._buf, self._snap, self._writable = [], guard, None, None, None

    # ---- placing (before the first pointer is taken) ----
    def _place(self, kind, shape, nb, per, bstride, align, skew, dtype, host):
        assert self._buf is None, "place every operand before taking the first pointer"
        assert align % 4 == 0 and align >= 4 and nb >= 1 and per >= 1
        bstride = per if bstride is None else int(bstride)
        assert bstride >= per or nb == 1, "samples would overlap"
        a = align // 4
        off = (self._cursor + a - 1) // a * a + skew
        r = Region(self, kind, off, shape, nb, per, bstride, dtype, host)
        self.regions.append(r)
        self._cursor = off + r.span + self.guard
        return r

    @staticmethod
    def _words_per(dtype):
        return {torch.float32: 1, torch.int32: 1, torch.int64: 2, torch.float64: 2}[dtype]

    def _split(self, shape, dtype, strided):
        shape = tuple(int(s) for s in shape) or (1,)
        n = int(np.prod(shape)) * self._words_per(dtype)
        nb = shape[0] if strided else 1
        return shape, nb, n // nb

    def place_input(self, t, bstride=None, align=16, skew=0):
        """Copies host tensor `t` in; with `bstride` its samples (dim 0) lie that many words apart, PATTERN in between.
        `skew` words are added to the aligned offset (an operand that is deliberately NOT `align`-aligned).
        A uint8 tensor (a mask) is one dense run of bytes padded to whole words, the padding bytes holding PATTERN's bytes."""
        t = t.detach().cpu().contiguous()
        if t.dtype == torch.uint8:
            assert bstride is None, "a byte operand is dense"
            n = t.numel()
            assert n >= 1
            host = torch.full(((n + 3) // 4,), PATTERN, dtype=torch.int32)
            host.view(torch.uint8)[:n] = t.reshape(-1)
            shape = tuple(int(s) for s in t.shape) or (1,)
            return self._place(_INPUT, shape, 1, host.numel(), None, align, skew, torch.uint8, host)
        shape, nb, per = self._split(t.shape, t.dtype, bstride is not None)
        return self._place(_INPUT, shape, nb, per, bstride, align, skew, t.dtype, t.reshape(-1).view(torch.int32).clone())

    def place_inout(self, t, bstride=None, align=16, skew=0):
        """An operand the call updates in place (running statistics, a step counter, the destination of an accumulating call):
        initial values from `t`, must end finite.  With `bstride` its samples (dim 0) lie that many words apart, PATTERN in between -
        gap words that must hold their bits like any other."""
        t = t.detach().cpu().contiguous()
        shape, nb, per = self._split(t.shape, t.dtype, bstride is not None)
        return self._place(_INOUT, shape, nb, per, bstride, align, skew, t.dtype, t.reshape(-1).view(torch.int32).clone())

    def place_output(self, shape, bstride=None, align=16, skew=0, written=True, dtype=torch.float32):
        """An output, PATTERN-prefilled.  written=False: the call is given NULL (or refuses) - the region must stay untouched."""
        shape, nb, per = self._split(shape, dtype, bstride is not None)
        return self._place(_OUTPUT if written else _ABSENT, shape, nb, per, bstride, align, skew, dtype, None)

    def place_ws(self, n, align=16, skew=0):
        """A workspace of exactly `n` floats, PATTERN-prefilled (a NaN: whatever is read before it is written poisons the result)."""
        return self._place(_WS, (int(n),), 1, int(n), None, align, skew, torch.float32, None)

    # ---- the buffer ----
    def _commit(self):
        total = self._cursor
        host = torch.full((total,), PATTERN, dtype=torch.int32)
        writable = torch.zeros(total, dtype=torch.bool)
        for r in self.regions:
            for k, (lo, hi) in enumerate(r.slices()):
                if r.kind in (_INPUT, _INOUT):
                    host[lo:hi] = r.host[k * (hi - lo):(k + 1) * (hi - lo)]
                if r.kind in (_OUTPUT, _WS, _INOUT):
                    writable[lo:hi] = True
        self._snap = host.to(self.device)
        self._writable = writable.to(self.device)
        self._buf = self._snap.clone()
        assert self._buf.data_ptr() % 16 == 0

    def buffer(self):
        if self._buf is None:
            self._commit()
        return self._buf

    def base_address(self):
        return self.buffer().data_ptr()

    def rearm(self, ws_fill=None):
        """Back to the state before the call; with `ws_fill` every workspace holds that finite constant instead of PATTERN."""
        self.buffer().copy_(self._snap)
        if ws_fill is not None:
            bits = int(np.float32(ws_fill).view(np.int32))
            for r in self.regions:
                if r.kind == _WS:
                    self._buf[r.offset:r.offset + r.per] = bits

    # ---- the check ----
    def violations(self):
        """A list of messages, empty when the call kept its contract."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        buf, out = self.buffer(), []
        touched = (buf != self._snap) & ~self._writable
        if bool(touched.any()):
            where = touched.nonzero().view(-1).cpu()
            out.append("%d words outside every output were written, first at word %d (%s)"
                       % (len(where), int(where[0]), self.describe(int(where[0]))))
        for i, r in enumerate(self.regions):
            if r.kind not in (_OUTPUT, _INOUT):
                continue
            w = r.words()
            unwritten = int((w == PATTERN).sum())
            if unwritten:
                out.append("%s #%d %s: %d of %d words never written" % (r.kind, i, r.shape, unwritten, w.numel()))
            elif r.dtype.is_floating_point and not bool(torch.isfinite(w.view(r.dtype)).all()):
                out.append("%s #%d %s holds non-finite values" % (r.kind, i, r.shape))
        return out

    def check(self):
        v = self.violations()
        assert not v, "; ".join(v)

    def describe(self, word):
        """Where a word of the arena lies, for a failure message."""
        for i, r in enumerate(self.regions):
            if r.offset - self.guard <= word < r.offset:
                return "%d words before %s #%d %s" % (r.offset - word, r.kind, i, r.shape)
            if r.offset <= word < r.offset + r.span:
                b, p = divmod(word - r.offset, r.bstride)
                return ("%s #%d %s sample %d word %d" if p < r.per else "the gap of %s #%d %s behind sample %d, stride word %d") % (
                    r.kind, i, r.shape, b, p)
            if r.offset + r.span <= word < r.offset + r.span + self.guard:
                return "%d words past the end of %s #%d %s" % (word - (r.offset + r.span) + 1, r.kind, i, r.shape)
        return "between operands"
