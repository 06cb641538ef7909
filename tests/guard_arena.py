"""Guard-band arena: every device buffer of ONE C-ABI call inside one torch.uint8 allocation, each buffer exactly as long as
the header says, a poisoned band right before and right after it.  The same layout code serves CPU tensors
(tests/test_guard_arena.py drives it with planted defects) and the GPU sweep (tests/test_gpu_guard_bands.py).

Layout of one buffer:   [alignment padding + guard band][buffer][guard band]
  - the band after a buffer starts at the very next byte; padding goes in FRONT of the leading band, never between a buffer
    and a band;
  - every band is at least GUARD = 256 KiB: a condition, not a measurement -- four times the largest tile one workgroup of
    any kernel here walks in one plane (16 384 float32 pixels = 64 KiB: the polynomial layers' coefficient-gradient tile of
    1024 x 16 steps; the streaming kernels own 4 096 pixels), so an overrun by a whole tile still lands in memory the test owns.

Alignment classes (the offset of a buffer modulo 16; the arena's base is on a 256-byte boundary):
  "16"    every buffer on the 16-byte grid: the float4 kernels are taken;
  "16+4"  float buffers 4 bytes past the grid (float64 ones 8, their natural alignment), byte buffers 1 byte past it -- what
          tests/test_gpu_parity.py's _misaligned() hands out: the one-element-per-lane kernels are taken.
  A buffer with `grid` set (workspaces and 16-byte scratches: 16; the 126-coefficient tables: 8) gets what the header demands
  in both classes: on the 16-byte grid in "16", `grid` bytes past it in "16+4" (16 past = on it).

Poison: two 32-bit words with no zero byte and no byte in common at any position.  A reads as a float32 NaN, B as a finite
float.  Guards, outputs, workspace and scratch are poisoned alike; inputs hold the test's data.

Checks (run_both), each reporting buffer, side and first offending byte offset through GuardError:
  guard       every guard byte is unchanged                      (side "before" / "after", offset relative to the buffer)
  input       every input buffer is unchanged
  inner       the `keep` ranges of an output (rows outside a slab) still hold their poison
  unwritten   no element of an ASSIGNED output still holds poison -- the poison of BOTH runs: a computed value may equal one
              pattern's word by chance (the finite one is a plausible pixel), never both
  poison      the call runs under A and under B on the same inputs: every output is bit-identical between the two runs (an
              element nobody wrote differs; so does a load from outside a buffer that reaches a result)
Workspace and scratch contents are exempt from the last two; their guards are not exempt from the first.
"""
import torch

GUARD = 256 * 1024
POISON_A = 0x7FC1A5C3  # float32 NaN
POISON_B = 0x3E5A7B9D  # float32 0.2133...
CLASSES = ("16", "16+4")

IN, OUT, INOUT, WORK = "in", "out", "inout", "work"


class GuardError(AssertionError):
    def __init__(self, check, buffer, side, offset, detail=""):
        self.check, self.buffer, self.side, self.offset = check, buffer, side, offset
        super().__init__(f"{check}: buffer '{buffer}' ({side}), first offending byte offset {offset}{detail}")


class Buf:
    """One buffer of the call.  role IN: `data` is the test's tensor.  OUT: `nbytes` (or shape + dtype) of poison, ASSIGNED by
    the call; `keep` = byte ranges [(lo, hi), ...] the call must leave alone.  INOUT: `data` is a set value the call updates
    (apply_curve's `reg`).  WORK: workspace / scratch of exactly `nbytes`, contents exempt.  grid: see the module docstring."""

    def __init__(self, name, role, data=None, nbytes=None, dtype=None, shape=None, grid=None, keep=()):
        self.name, self.role, self.grid, self.keep = name, role, grid, tuple(keep)
        if data is not None:
            data = data.contiguous()
            dtype, shape = data.dtype, tuple(data.shape)
            nbytes = data.numel() * data.element_size()
        elif shape is not None:
            n = 1
            for s in shape:
                n *= s
            nbytes = n * _itemsize(dtype)
            shape = tuple(shape)
        self.data, self.nbytes, self.dtype, self.shape = data, int(nbytes), dtype or torch.uint8, shape
        self.itemsize = _itemsize(self.dtype)
        assert self.nbytes > 0 and self.nbytes % self.itemsize == 0, (name, nbytes)


def _itemsize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def skew_of(cls, itemsize, grid=None):
    """The offset modulo 16 a buffer of this class starts at."""
    assert cls in CLASSES, cls
    if cls == "16":
        return 0
    if grid is not None:
        return grid % 16
    return 1 if itemsize == 1 else max(4, itemsize)


class Layout:
    """Byte offsets of every buffer and band; plain integers, no tensor."""

    def __init__(self, bufs, cls, guard=GUARD):
        self.cls, self.guard, self.bufs = cls, guard, {b.name: b for b in bufs}
        assert len(self.bufs) == len(bufs), "duplicate buffer name"
        self.off, self.before, self.after = {}, {}, {}
        cur = 0
        for b in bufs:
            skew = skew_of(cls, b.itemsize, b.grid)
            off = cur + guard
            off += (skew - off) % 16
            self.before[b.name] = (cur, off)             # padding + band, ends at the buffer's first byte
            self.off[b.name] = off
            self.after[b.name] = (off + b.nbytes, off + b.nbytes + guard)  # starts at the very next byte
            cur = off + b.nbytes + guard
        self.total = cur

    def regions(self):
        """Every region in address order: (lo, hi, buffer name, side)."""
        out = []
        for n, b in self.bufs.items():
            out += [(*self.before[n], n, "before"), (self.off[n], self.off[n] + b.nbytes, n, "buffer"), (*self.after[n], n, "after")]
        return out


def _poison_bytes(word, total, device):
    w = torch.tensor([word - (1 << 32) if word >= (1 << 31) else word], dtype=torch.int32)
    return w.repeat((total + 3) // 4).view(torch.uint8)[:total].to(device)


class Arena:
    def __init__(self, bufs, cls, device, word, guard=GUARD):
        self.layout = L = Layout(bufs, cls, guard)
        self.device = torch.device(device)
        raw = torch.empty(L.total + 256, dtype=torch.uint8, device=self.device)
        shift = (-raw.data_ptr()) % 256
        self._raw = raw
        self.bytes = raw[shift:shift + L.total]
        assert self.bytes.data_ptr() % 256 == 0
        self.poison = _poison_bytes(word, L.total, self.device)  # word grid anchored at the arena's base
        self.bytes.copy_(self.poison)
        for b in bufs:
            if b.data is not None:
                self._slice(b.name).copy_(b.data.reshape(-1).view(torch.uint8).to(self.device))
        self.initial = self.bytes.clone()

    def _slice(self, name):
        o = self.layout.off[name]
        return self.bytes[o:o + self.layout.bufs[name].nbytes]

    def has(self, name):
        return name in self.layout.bufs

    def off(self, name):
        return self.layout.off[name]

    def nbytes(self, name):
        """The size the call is given for a workspace / scratch: exactly the buffer's length (0 if absent)."""
        return self.layout.bufs[name].nbytes if self.has(name) else 0

    def ptr(self, name):
        """The device address of a buffer; 0 (NULL) for a buffer the case left out."""
        return self.bytes.data_ptr() + self.layout.off[name] if self.has(name) else 0

    def read(self, name):
        """A copy of the buffer's current contents in its own dtype and shape."""
        b = self.layout.bufs[name]
        t = self._slice(name).clone().view(b.dtype)
        return t.view(b.shape) if b.shape is not None else t

    def write(self, name, tensor):
        """(for the CPU stand-ins) store a tensor of the buffer's dtype at the buffer's start"""
        flat = tensor.contiguous().reshape(-1).view(torch.uint8)
        o = self.layout.off[name]
        self.bytes[o:o + flat.numel()].copy_(flat)

    def outputs(self):
        return [n for n, b in self.layout.bufs.items() if b.role in (OUT, INOUT)]

    def check(self):
        """guard, input and inner, in this order; raises GuardError at the first finding."""
        L = self.layout
        diff = self.bytes != self.initial
        for n, b in L.bufs.items():  # what the call may write
            if b.role == IN:
                continue
            o = L.off[n]
            allowed = torch.ones(b.nbytes, dtype=torch.bool, device=self.device)
            for lo, hi in b.keep:
                allowed[lo:hi] = False
            diff[o:o + b.nbytes] &= ~allowed
        if bool(diff.any()):
            first = int(torch.nonzero(diff)[0])
            for lo, hi, n, side in L.regions():
                if lo <= first < hi:
                    o = L.off[n]
                    if side == "buffer":
                        kind = "input" if L.bufs[n].role == IN else "inner"
                        raise GuardError(kind, n, "inner" if kind == "inner" else "buffer", first - o)
                    raise GuardError("guard", n, side, first - o if side == "before" else first - (o + L.bufs[n].nbytes),
                                     " (relative to the buffer's first byte)" if side == "before" else " (past the buffer's last byte)")
            raise AssertionError(first)

    def stale(self, name):
        """-> (mask, bytes per entry): the elements of an output that hold this arena's poison (outside the `keep` ranges)."""
        b, o = self.layout.bufs[name], self.layout.off[name]
        eq = self.bytes[o:o + b.nbytes] == self.poison[o:o + b.nbytes]
        for lo, hi in b.keep:
            eq[lo:hi] = False
        if b.itemsize >= 4:
            return eq.view(-1, b.itemsize).all(1), b.itemsize
        if b.nbytes >= 4:  # bytes: one byte equals its poison by chance once in 256; four in a row do not
            return eq[:-3] & eq[1:-2] & eq[2:-1] & eq[3:], 1
        return eq.all().reshape(1), 1


def run_both(bufs, cls, device, call, guard=GUARD):
    """The call under poison A and under poison B, same inputs; every check of the module docstring.
    call(arena) makes the call (and asserts its return code).  -> the arena of the pattern-A run."""
    arenas = []
    for word in (POISON_A, POISON_B):
        a = Arena(bufs, cls, device, word, guard)
        call(a)
        if a.device.type == "cuda":
            torch.cuda.synchronize(a.device)
        a.check()
        arenas.append(a)
    A, B = arenas
    for n, b in A.layout.bufs.items():
        if b.role != OUT:
            continue
        # unwritten = holds the poison of BOTH runs (a computed value that happens to equal one pattern's word -- the finite one
        # is a plausible pixel -- does not equal the other's)
        (sa, scale), (sb, _) = A.stale(n), B.stale(n)
        both = sa & sb
        if bool(both.any()):
            raise GuardError("unwritten", n, "buffer", int(torch.nonzero(both)[0]) * scale)
    for n in A.outputs():
        b = A.layout.bufs[n]
        o = A.layout.off[n]
        ne = A.bytes[o:o + b.nbytes] != B.bytes[o:o + b.nbytes]
        for lo, hi in b.keep:
            ne[lo:hi] = False
        if bool(ne.any()):
            first = int(torch.nonzero(ne)[0]) // b.itemsize * b.itemsize  # (the element's first byte)
            raise GuardError("poison", n, "buffer", first, ": the result depends on the poison pattern")
    return A
