"""A guarded arena for the memory-contract tests (no tests in here; tests/test_arena.py proves the instrument on the CPU,
tests/test_memory_contract.py uses it on the GPU).

One uint8 tensor filled with the byte 0xFF -- NaN in fp32, bf16 and e4m3fn, -1 in int32 -- out of which a test carves every tensor of a
call: at a chosen residue of the address, with at least BAND untouched bytes before and after each and TAIL untouched bytes behind the
last.  `check()` then reads the WHOLE arena back: a byte that belongs to no writable view must still be 0xFF, a view that was only an
input must still hold what `load()` put there, bit for bit.  So the arena shows, in one pass,

  * a store outside a tensor (before it, behind it, or far behind it: the whole arena is compared, not only the bands),
  * a store into an input,
  * a read of memory the call did not own or did not write first: it reads NaN, which the caller's comparison of results shows.

Residues.  `carve(..., residue=(r, m))` places the view at an address that is r modulo m.  OFFSET is 16 mod 256, the least the library
accepts for a base pointer and nothing more; SIDE is 4 mod 16, for the int32 / fp32 side inputs; ALIGNED is 0 mod 512, what a caching
allocator hands out.  Views are `arena[a:b].view(dtype).view(shape)`, or `as_strided` over the same bytes when strides (in elements) are
given -- the gaps such strides leave inside [a, b) belong to no view and are checked like a band.
"""
import math

import torch

BAND = 4096            # untouched bytes before and after every view, at least
TAIL = 1 << 20         # untouched bytes behind the last view
FILL = 0xFF
ALIGNED, OFFSET, SIDE = (0, 512), (16, 256), (4, 16)
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """`t` as integers of its element size (any strides): comparisons and copies of bit patterns, NaNs and fp8 included"""
    return t if t.dtype in _BITS.values() else t.view(_BITS[t.element_size()])


def itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def extent(shape, strides=None):
    """elements from the first to one past the last element of a view (dense when strides is None)"""
    if strides is None:
        return math.prod(shape)
    assert len(strides) == len(shape) and all(n >= 1 for n in shape) and all(s >= 0 for s in strides)
    return sum((n - 1) * s for n, s in zip(shape, strides)) + 1


def footprint(shape, dtype, residue=OFFSET, strides=None):
    """bytes an arena sets aside for one carving: its extent, a band, and the most its residue can cost"""
    return extent(shape, strides) * itemsize(dtype) + BAND + residue[1]


class ArenaError(AssertionError):
    """`check()` found a byte that is not what it must be.  name: the nearest carved tensor; offset: the byte's offset from that
    tensor's first byte (negative: before it; >= nbytes: behind it); nbytes: that tensor's extent; kind: "outside" (a byte that
    belongs to no writable view) or "input" (a byte of a view that was only an input)"""

    def __init__(self, name, offset, nbytes, kind, got, want, count):
        where = f"{-offset} bytes before its start" if offset < 0 else \
            f"{offset - nbytes + 1} bytes past its end" if offset >= nbytes else "inside it"
        super().__init__(f"arena: {count} bytes changed that the call does not own; the first is at offset {offset:+d} of '{name}' "
                         f"({where}; {'an input was written' if kind == 'input' else 'outside every writable view'}): "
                         f"0x{got:02X}, was 0x{want:02X}")
        self.name, self.offset, self.nbytes, self.kind, self.count = name, offset, nbytes, kind, count


class Carving:
    def __init__(self, name, a, nbytes, dtype, shape, strides, writable):
        self.name, self.a, self.nbytes, self.dtype, self.shape, self.strides, self.writable = name, a, nbytes, dtype, shape, strides, writable
        self.copy = None

    def of(self, flat, raw=False):
        """this carving's view of a uint8 tensor laid out like the arena; raw: as integers of the element size (bits())"""
        base = flat[self.a:self.a + self.nbytes]
        dt = _BITS[itemsize(self.dtype)] if raw else self.dtype
        base = base.view(dt) if dt != torch.uint8 else base
        return base.view(self.shape) if self.strides is None else torch.as_strided(base, self.shape, self.strides)


class Arena:
    """`Arena(device, room)`: room = the sum of `footprint()` over the carvings to come; the arena holds room + TAIL bytes.
    `Arena.of(device, specs)` sizes and carves in one step."""

    def __init__(self, device, room):
        self.size = BAND + int(room) + TAIL
        raw = torch.full((self.size + 512,), FILL, dtype=torch.uint8, device=device)
        shift = -raw.data_ptr() % 512
        self.bytes = raw[shift:shift + self.size]          # the arena's own base is 512-byte aligned
        self.base = self.bytes.data_ptr()
        self.cursor = BAND
        self.carvings = []

    @classmethod
    def of(cls, device, specs):
        """specs: {name: dict(shape=, dtype=, residue=, strides=, writable=)} -> (arena, {name: view})"""
        specs = {n: dict(s) for n, s in specs.items()}
        arena = cls(device, sum(footprint(s["shape"], s["dtype"], s.get("residue", OFFSET), s.get("strides")) for s in specs.values()))
        return arena, {n: arena.carve(name=n, **s) for n, s in specs.items()}

    def carve(self, shape, dtype, residue=OFFSET, strides=None, writable=False, name=None):
        r, m = residue
        isz = itemsize(dtype)
        assert 0 <= r < m and r % isz == 0, f"residue {residue} cannot hold {dtype}"
        shape = tuple(int(n) for n in shape)
        strides = None if strides is None else tuple(int(s) for s in strides)
        nbytes = extent(shape, strides) * isz
        a = self.cursor + (r - (self.base + self.cursor)) % m
        assert a + nbytes + TAIL <= self.size, "arena too small: size it with footprint()"
        c = Carving(name or f"#{len(self.carvings)}", a, nbytes, dtype, shape, strides, bool(writable))
        self.carvings.append(c)
        self.cursor = a + nbytes + BAND
        view = c.of(self.bytes)
        assert view.data_ptr() % m == r and view.data_ptr() == self.base + a
        return view

    def _carving(self, view):
        a = view.data_ptr() - self.base
        for c in self.carvings:
            if c.a == a:
                return c
        raise KeyError("not a view this arena carved")

    def load(self, view, cpu_tensor):
        """copy `cpu_tensor` (the view's shape and dtype) into the view and keep it: `check()` holds a non-writable view to it"""
        c = self._carving(view)
        assert tuple(cpu_tensor.shape) == c.shape and cpu_tensor.dtype == c.dtype and cpu_tensor.device.type == "cpu"
        c.copy = bits(cpu_tensor).clone()
        bits(view).copy_(c.copy)
        return view

    def refill(self, view):
        """0xFF over a writable view again (between two calls that write the same outputs)"""
        c = self._carving(view)
        assert c.writable
        b = bits(view)
        b.fill_(FILL if b.dtype == torch.uint8 else -1)

    def check(self):
        """every byte outside the writable views is 0xFF, or what `load()` put there; raises ArenaError at the first that is not"""
        got = self.bytes.cpu()
        want = torch.full((self.size,), FILL, dtype=torch.uint8)
        free = torch.zeros(self.size, dtype=torch.uint8)         # 0xFF on the bytes of writable views: anything may stand there
        for c in self.carvings:
            if c.copy is not None:
                c.of(want, raw=True).copy_(c.copy)
        for c in self.carvings:
            if c.writable:
                c.of(free, raw=True).fill_(FILL if itemsize(c.dtype) == 1 else -1)
        bad = (got != want) & (free == 0)
        count = int(bad.sum())
        if not count:
            return
        at = int(bad.int().argmax())
        gap = lambda c: 0 if c.a <= at < c.a + c.nbytes else min(abs(at - c.a), abs(at - (c.a + c.nbytes - 1)))
        c = min(self.carvings, key=gap)
        kind = "input" if gap(c) == 0 and not c.writable else "outside"
        raise ArenaError(c.name, at - c.a, c.nbytes, kind, int(got[at]), int(want[at]), count)
