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

Operands of 2-byte elements (the reduced-precision path) are guarded element by element: PATTERN16 is a NaN in bf16 and in f16 that
no conversion produces (theirs are 0x7FC0 / 0x7E00).

    img = a.place_lp(torch.bfloat16, B, H, W, cpitch, reads=[(0, x)], writes=[(32, 32)])   # an lp image [B][H+2][W+2][cpitch]
    pk = a.place_output16(n, torch.bfloat16)                                               # a dense pack of n elements
    m = a.place_output_u8((B, T))                                                          # a byte output, padded to whole words
    img = a.place_output_u8((n,), lead=1, expect=ref)                                      # ... one byte off a word, of any byte values
    src = a.place_input_u8(image, lead=3)                                                  # a byte input three bytes off a word
    tmp = a.place_ws_u8(n, lead=2)                                                         # a workspace of exactly n BYTES
    img = a.place_inout_u8(prior, lead=1, may=owned, expect=ref)                           # a byte image with prior contents, partly owned
    out = a.place_masked(base, may=owned)                                                  # a float32 output only `may` of which is the call's

An lp image holds zeros on its one-pixel border, the values of `reads` (NCHW tensors, exactly representable) in their channel
ranges and PATTERN16 in every other channel of the interior; the call may write the interior pixels x the channel ranges of
`writes` and nothing else, and must leave no PATTERN16 and only finite values there.
"""
import ctypes

import numpy as np
import torch

PATTERN = 0x7FC5A5A5
PATTERN16 = 0x7FC5        # per 2-byte element
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
        return self.arena.base_address() + 4 * self.offset + getattr(self, "lead", 0)     # lead: bytes, Region16 only

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

    # what _commit needs of a region: its initial words and which of their bits the call may change
    def initial(self, k, n):
        """(words or None = PATTERN, writable bit mask) of run `k` (`n` words) of slices()."""
        words = self.host[k * n:(k + 1) * n] if self.kind in (_INPUT, _INOUT) else None
        return words, (-1 if self.kind in (_OUTPUT, _WS, _INOUT) else 0)

    def refill(self, bits):
        """A workspace-like operand before the second of two calls: every writable word holds `bits` (a finite float)."""
        if self.kind == _WS:
            self.arena.buffer()[self.offset:self.offset + self.per] = bits

    def complaints(self, i):
        if self.kind not in (_OUTPUT, _INOUT):
            return []
        w = self.words()
        unwritten = int((w == PATTERN).sum())
        if unwritten:
            return ["%s #%d %s: %d of %d words never written" % (self.kind, i, self.shape, unwritten, w.numel())]
        if self.dtype.is_floating_point and not bool(torch.isfinite(w.view(self.dtype)).all()):
            return ["%s #%d %s holds non-finite values" % (self.kind, i, self.shape)]
        return []


class RegionMasked(Region):
    """A dense float32 operand whose elements the call may write only where `may` holds: `host` holds its initial words (PATTERN
    where the caller gave no base), `must` the elements that have to be written - those it may write that start as PATTERN."""

    def __init__(self, arena, offset, shape, host, may):
        super().__init__(arena, _INOUT, offset, shape, 1, host.numel(), host.numel(), torch.float32, host)
        self.may = may
        self.must = may & (host == PATTERN)

    def initial(self, k, n):
        return self.host, torch.where(self.may, torch.tensor(-1, dtype=torch.int32), torch.tensor(0, dtype=torch.int32))

    def complaints(self, i):
        w = self.words()
        unwritten = int(((w == PATTERN) & self.must).sum())
        if unwritten:
            return ["%s #%d %s: %d of %d elements never written" % (self.kind, i, self.shape, unwritten, int(self.must.sum()))]
        if not bool(torch.isfinite(w.view(torch.float32)[self.may]).all()):
            return ["%s #%d %s holds non-finite values" % (self.kind, i, self.shape)]
        return []


def _pattern16(n):
    return torch.full((n,), PATTERN16, dtype=torch.int16)


class Region16(Region):
    """A dense run of 2-byte elements (a weight pack, att_pack) or of bytes (a mask), padded to whole words; `image` holds its initial
    elements, `mask` which of them the call may write (all ones / zero per element), `must` which of those it has to write."""

    def __init__(self, arena, kind, offset, shape, dtype, image, mask, must, finite, lead=0):
        self.image, self.mask, self.must, self.finite, self.lead = image, mask, must, finite, lead
        super().__init__(arena, kind, offset, shape, 1, image.view(torch.int32).numel(), None, dtype, None)
        self.bstride = self.per

    def initial(self, k, n):
        return self.image.view(torch.int32), self.mask.view(torch.int32)

    def refill(self, bits):
        """Outputs of 2-byte elements count as workspace-like: an element the call never writes then differs between the two calls."""
        if self.kind == _ABSENT or self.image.dtype != torch.int16:
            return
        fill = torch.tensor([1.5]).to(self.dtype if self.dtype.is_floating_point else torch.float16).view(torch.int16)
        img = torch.where(self.must, fill.expand_as(self.image), self.image)
        self.arena.buffer()[self.offset:self.offset + self.per] = img.view(torch.int32).to(self.arena.device)

    def elements(self):
        """The operand's elements as they are now (int16 or uint8, flat, padding included), on the host."""
        return self.words().view(self.image.dtype)

    def read(self):
        lead = self.lead // self.image.dtype.itemsize
        e = self.elements()[lead:lead + int(np.prod(self.shape))].reshape(self.shape).clone()
        return e.view(self.dtype) if self.image.dtype == torch.int16 and self.dtype.itemsize == 2 else e

    def complaints(self, i):
        if self.kind == _ABSENT:
            return []
        e = self.elements()
        unwritten = int(((e == self.image) & self.must).sum())
        if unwritten:
            return ["%s #%d %s: %d of %d elements never written" % (self.kind, i, self.shape, unwritten, int(self.must.sum()))]
        if self.finite and not bool(torch.isfinite(e.view(self.dtype)[self.must]).all()):
            return ["%s #%d %s holds non-finite values" % (self.kind, i, self.shape)]
        return []


class LpImage(Region16):
    """A zero-bordered channels-last image [B][H+2][W+2][cpitch] of 2-byte elements."""

    def __init__(self, arena, offset, dtype, B, H, W, cpitch, reads, writes, written):
        img = torch.zeros(B, H + 2, W + 2, cpitch, dtype=torch.int16)
        inner = img[:, 1:-1, 1:-1]
        inner[:] = PATTERN16
        mask, must = torch.zeros_like(img), torch.zeros(img.shape, dtype=torch.bool)
        for coff, t in reads:
            t = t.detach().cpu().float()
            assert t.shape[0] == B and t.shape[2:] == (H, W) and 0 <= coff and coff + t.shape[1] <= cpitch
            assert torch.equal(t.to(dtype).float(), t), "an input of an lp image is exactly representable in its type"
            inner[..., coff:coff + t.shape[1]] = t.permute(0, 2, 3, 1).to(dtype).view(torch.int16)
        for coff, c in (writes if written else ()):
            assert 0 <= coff and coff + c <= cpitch
            mask[:, 1:-1, 1:-1, coff:coff + c] = -1
            must[:, 1:-1, 1:-1, coff:coff + c] = True
        for coff, t in reads:                                     # a channel read AND written starts from its input: nothing to find there
            must[:, 1:-1, 1:-1, coff:coff + t.shape[1]] = False
        self.B, self.H, self.W, self.cpitch = B, H, W, cpitch
        kind = _INOUT if (reads and writes) else _OUTPUT if writes else _INPUT
        if writes and not written:
            kind = _ABSENT
        super().__init__(arena, kind, offset, (B, H + 2, W + 2, cpitch), dtype, img.reshape(-1), mask.reshape(-1), must.reshape(-1), True)

    def nchw(self, coff, c):
        """Channels [coff, coff + c) of the interior as fp32 [B][c][H][W]."""
        e = self.elements().reshape(self.shape)[:, 1:-1, 1:-1, coff:coff + c]
        return e.contiguous().view(self.dtype).float().permute(0, 3, 1, 2).contiguous()


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

    def _place16(self, region, align, skew):
        assert self._buf is None, "place every operand before taking the first pointer"
        a = align // 4
        region.offset = (self._cursor + a - 1) // a * a + skew
        self.regions.append(region)
        self._cursor = region.offset + region.span + self.guard
        return region

    def place_lp(self, dtype, B, H, W, cpitch, reads=(), writes=(), align=16, skew=0, written=True):
        """An lp image: `reads` = [(coff, values [B][C][H][W])], `writes` = [(coff, C)] - an input, an output or, with both, an in/out
        operand.  written=False: the call refuses - nothing of it may change."""
        assert (B * (H + 2) * (W + 2) * cpitch) % 2 == 0
        return self._place16(LpImage(self, 0, dtype, B, H, W, cpitch, list(reads), list(writes), written), align, skew)

    def _dense16(self, kind, shape, dtype, values, written, finite, align, skew):
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape))
        img = _pattern16(n + (n & 1))
        if values is not None:
            img[:n] = values.reshape(-1)
        mask, must = torch.zeros_like(img), torch.zeros(img.shape, dtype=torch.bool)
        if kind == _OUTPUT:
            mask[:n], must[:n] = -1, True
        return self._place16(Region16(self, kind if written else _ABSENT, 0, shape, dtype, img, mask, must, finite), align, skew)

    def place_input16(self, t, align=16, skew=0):
        """A dense operand of 2-byte elements (bf16 / f16 / int16 tensor) the call only reads."""
        t = t.detach().cpu().contiguous()
        assert t.dtype.itemsize == 2
        return self._dense16(_INPUT, t.shape, t.dtype, t.view(torch.int16), True, False, align, skew)

    def place_output16(self, shape, dtype, align=16, skew=0, written=True, finite=True):
        """A dense output of 2-byte elements, PATTERN16-prefilled; finite=False: raw bits (att_pack's mask words)."""
        return self._dense16(_OUTPUT, shape, dtype, None, written, finite, align, skew)

    def place_output_u8(self, shape, align=16, skew=0, written=True, lead=0, expect=None):
        """A byte output (the text tail's mask): PATTERN's bytes before the call - none of them 0 or 1 - and behind its last element.
        `lead` (0..3): the operand starts that many BYTES behind the word `align` and `skew` place, the bytes in front of it guarded
        like those behind its last element (an output that is not word aligned).  `expect` (uint8, the right result): an output
        whose values may be any byte (an image; 0xA5, 0xC5 and 0x7F are PATTERN's) counts as unwritten only where the byte it holds
        after the call is PATTERN's and the right one is another."""
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape))
        assert 0 <= lead <= 3
        img = torch.full(((lead + n + 3) // 4,), PATTERN, dtype=torch.int32).view(torch.uint8).clone()
        mask, must = torch.zeros_like(img), torch.zeros(img.shape, dtype=torch.bool)
        mask[lead:lead + n], must[lead:lead + n] = 255, True
        if expect is not None:
            must[lead:lead + n] = expect.reshape(-1) != img[lead:lead + n]
        return self._place16(Region16(self, _OUTPUT if written else _ABSENT, 0, shape, torch.uint8, img, mask, must, False, lead),
                             align, skew)

    def place_input_u8(self, t, align=16, skew=0, lead=0):
        """A byte input (an image) the call only reads, starting `lead` (0..3) BYTES behind the word `align` and `skew` place: the
        bytes in front of it and behind its last element hold PATTERN's and are guarded like every byte of the operand itself."""
        t = t.detach().cpu().contiguous()
        assert t.dtype == torch.uint8 and t.numel() >= 1 and 0 <= lead <= 3
        n = t.numel()
        img = torch.full(((lead + n + 3) // 4,), PATTERN, dtype=torch.int32).view(torch.uint8).clone()
        img[lead:lead + n] = t.reshape(-1)
        mask, must = torch.zeros_like(img), torch.zeros(img.shape, dtype=torch.bool)
        shape = tuple(int(s) for s in t.shape) or (1,)
        return self._place16(Region16(self, _INPUT, 0, shape, torch.uint8, img, mask, must, False, lead), align, skew)

    def place_inout_u8(self, t, align=16, skew=0, lead=0, may=None, expect=None):
        """A byte operand with prior contents `t` that the call writes in part (an image of which only owned rectangles are the
        call's): `may` (bool, t's shape; all of it when None) says which bytes it may change, every other byte - and those in front
        of the operand and behind it - must hold its bits.  `expect` (uint8, the right result): a byte the call may write counts as
        unwritten where it still holds its prior value and the right one is another."""
        t = t.detach().cpu().contiguous()
        assert t.dtype == torch.uint8 and t.numel() >= 1 and 0 <= lead <= 3
        n = t.numel()
        img = torch.full(((lead + n + 3) // 4,), PATTERN, dtype=torch.int32).view(torch.uint8).clone()
        img[lead:lead + n] = t.reshape(-1)
        mask, must = torch.zeros_like(img), torch.zeros(img.shape, dtype=torch.bool)
        may = torch.ones(n, dtype=torch.bool) if may is None else may.reshape(-1).bool()
        assert may.numel() == n
        mask[lead:lead + n] = torch.where(may, 255, 0).to(torch.uint8)
        if expect is not None:
            must[lead:lead + n] = may & (expect.reshape(-1) != t.reshape(-1))
        shape = tuple(int(s) for s in t.shape) or (1,)
        return self._place16(Region16(self, _INOUT, 0, shape, torch.uint8, img, mask, must, False, lead), align, skew)

    def place_masked(self, base, may, align=16, skew=0):
        """A float32 output of which the call owns only the elements where `may` (bool, base's shape) holds: `base` (float32, finite)
        is what it holds before the call, or a shape - then PATTERN, and every element of `may` has to be written.  An element
        outside `may` must hold its bits (a hole no tile owns, the block of a window the kernels skip)."""
        assert self._buf is None, "place every operand before taking the first pointer"
        if torch.is_tensor(base):
            base = base.detach().cpu().contiguous()
            assert base.dtype == torch.float32
            shape, host = tuple(base.shape), base.reshape(-1).view(torch.int32).clone()
        else:
            shape = tuple(int(s) for s in base)
            host = torch.full((int(np.prod(shape)),), PATTERN, dtype=torch.int32)
        may = may.reshape(-1).bool()
        assert may.numel() == host.numel() >= 1
        a = align // 4
        r = RegionMasked(self, (self._cursor + a - 1) // a * a + skew, shape, host, may)
        self.regions.append(r)
        self._cursor = r.offset + r.span + self.guard
        return r

    def place_ws_u8(self, n, align=16, skew=0, lead=0):
        """A workspace of exactly `n` BYTES, `lead` bytes off a word, holding PATTERN's bytes: the call may write those n bytes, all
        of them or some, and not the byte in front of them nor the one behind."""
        n = int(n)
        assert n >= 1 and 0 <= lead <= 3
        img = torch.full(((lead + n + 3) // 4,), PATTERN, dtype=torch.int32).view(torch.uint8).clone()
        mask, must = torch.zeros_like(img), torch.zeros(img.shape, dtype=torch.bool)
        mask[lead:lead + n] = 255
        return self._place16(Region16(self, _WS, 0, (n,), torch.uint8, img, mask, must, False, lead), align, skew)

    def place_ws(self, n, align=16, skew=0):
        """A workspace of exactly `n` floats, PATTERN-prefilled (a NaN: whatever is read before it is written poisons the result)."""
        return self._place(_WS, (int(n),), 1, int(n), None, align, skew, torch.float32, None)

    # ---- the buffer ----
    def _commit(self):
        total = self._cursor
        host = torch.full((total,), PATTERN, dtype=torch.int32)
        writable = torch.zeros(total, dtype=torch.int32)           # per word, the bits the call may change
        for r in self.regions:
            for k, (lo, hi) in enumerate(r.slices()):
                words, mask = r.initial(k, hi - lo)
                if words is not None:
                    host[lo:hi] = words
                writable[lo:hi] = mask
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
                r.refill(bits)

    # ---- the check ----
    def violations(self):
        """A list of messages, empty when the call kept its contract."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        buf, out = self.buffer(), []
        touched = ((buf ^ self._snap) & ~self._writable) != 0
        if bool(touched.any()):
            where = touched.nonzero().view(-1).cpu()
            out.append("%d words outside every output were written, first at word %d (%s)"
                       % (len(where), int(where[0]), self.describe(int(where[0]))))
        for i, r in enumerate(self.regions):
            out.extend(r.complaints(i))
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
