"""Reference and scaffolding shared by the K/V cache append tests (tests/test_kv_append_abi.py on the CPU, tests/test_kv_append.py,
test_kv_append_varlen.py and the rope append tests on the GPU; no tests in here).  Plain torch on the CPU.

Writer.  `append()` is the contract of include/flash_attention.h (flash_attention_kv_append, _paged) spelled out: the position rule
(`positions()`), the value rule (`encode()`: a bit copy for a bf16 cache, `kv_cache_check.quantise`'s expression with a GIVEN descale
for an fp8 one), contiguous or paged, table entries outside [0, P) skipped.  Caches are handled as integer tensors -- uint8 for
e4m3fn bytes, int16 for bf16 patterns -- so that comparisons are of bits and NaN patterns compare like any other.

Yardstick of the yardstick.  `nearest_even_code()` finds the e4m3fn code of a quotient by brute force over the table of all codes
built from the format's definition (format_probe.TABLE): nearest value, ties to the even code, the sign kept, saturation at 448.
tests/test_kv_append_abi.py holds `encode()` against it on every bf16 bit pattern.

Scaffolding.  `sentinel()`: a cache pre-filled with a finite pattern (`SENT`), compared whole afterwards; `as_cache()`: the integer
tensor as the call takes it; `new_rows()`: the rows to append, special values among them; `descales()`; `same()`.
"""
import torch

from format_probe import TABLE

F8 = getattr(torch, "float8_e4m3fn", None)
bf, i16, u8 = torch.bfloat16, torch.int16, torch.uint8
SENT = {u8: 0xA5, i16: 0x5A5A}        # (0xA5 is a finite e4m3fn code, 0x5A5A a finite bf16: never what a NaN compares as)


def sentinel(shape, fp8, device="cpu"):
    dt = u8 if fp8 else i16
    return torch.full(shape, SENT[dt], dtype=dt, device=device)


def as_cache(t):
    """the integer tensor as the call takes it"""
    return t.view(F8) if t.dtype == u8 else t.view(bf)


def new_rows(shape, seed):
    """bf16 N(0, 1) scaled so that some values saturate at descales near 1 / 64, with the special values among them"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * 3).to(bf)
    flat = x.reshape(-1)
    special = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0, 0.0, 1e-30, -1e-30, 448.0, 464.0, 3e38], dtype=bf)
    flat[:special.numel()] = special
    flat[-special.numel():] = special.flip(0)
    return x


def descales(seed, fp8, Hkv=2):
    """(k_descale, v_descale) fp32 [Hkv] on the CPU, near 1 / 64 and near 1; (None, None) for a bf16 cache"""
    if not fp8:
        return None, None
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(Hkv, generator=g) * 0.05 + 0.01).float(), (torch.rand(Hkv, generator=g) * 2 + 0.5).float()


def all_bf16_patterns():
    """bf16 [65536]: element n has the bit pattern n"""
    return torch.arange(65536, dtype=torch.int32).to(i16).view(torch.bfloat16)


def positions(L, Sq, cap):
    """[(i, p)]: new row i of a sequence whose length (the new rows counted) is L goes to key position p"""
    L = min(int(L), cap)
    if L <= 0:
        return []
    return [(i, L - Sq + i) for i in range(Sq) if L - Sq + i >= 0]


def encode(x, ds, fp8):
    """x bf16 [B, Hkv, rows, d] (K/V heads in dimension 1) -> what the cache stores: int16 bit patterns, or (fp8) uint8 e4m3fn
    bytes of clamp(fp32(x) / ds[kvh], -448, 448); ds fp32 [Hkv] or None = 1"""
    assert x.dtype == torch.bfloat16
    if not fp8:
        return x.contiguous().view(i16)
    ds = torch.ones(x.shape[1]) if ds is None else ds.float().cpu()
    return (x.float() / ds[None, :, None, None]).clamp(-448, 448).to(F8).view(u8)


def append(new, cache, lens, ds=None, table=None):
    """A copy of `cache` with the rows of `new` (bf16 [B, Hkv, Sq, d]) appended.  cache: int16 (bf16 patterns) or uint8 (e4m3fn
    bytes), [B, Hkv, cap, d], or with `table` (int [B, max_pages], any values) a pool [P, Hkv, page, d].  lens: B ints or None"""
    out = cache.clone()
    B, _, Sq, _ = new.shape
    enc = encode(new, ds, cache.dtype == u8)
    page = cache.shape[2]
    cap = page * table.shape[1] if table is not None else cache.shape[2]
    for b in range(B):
        for i, p in positions(cap if lens is None else lens[b], Sq, cap):
            if table is None:
                out[b, :, p] = enc[b, :, i]
            else:
                e = int(table[b, p // page])
                if 0 <= e < cache.shape[0]:
                    out[e, :, p % page] = enc[b, :, i]
    return out


def quotient(x, ds):
    """the correctly rounded fp32 quotient fp32(x) / ds as float64: fp32 operands divided in float64 and rounded once to fp32 (53 >=
    2 * 24 + 2 bits: the double rounding is innocuous)"""
    d = float(torch.tensor(ds, dtype=torch.float32))
    return (x.double() / d).float().double()


def nearest_even_code(q):
    """float64 tensor of quotients -> (uint8 codes, bool is_nan): for every q that is not NaN the e4m3fn code nearest to
    clamp(q, -448, 448), found by search over TABLE; a tie goes to the code whose last bit is 0; the sign bit is q's own, also on
    zero.  Where q is NaN the code is 0x7F and is_nan says so (any NaN code is right there)"""
    flat = q.reshape(-1)
    mags = TABLE[:0x7F]                                          # the 127 finite non-negative codes, ascending
    assert bool((mags[1:] > mags[:-1]).all()) and float(mags[-1]) == 448.0
    nan = torch.isnan(flat)
    m = torch.where(nan, torch.zeros_like(flat), flat.abs().clamp(max=448.0))
    out = torch.empty(flat.shape, dtype=u8)
    even = (torch.arange(0x7F) & 1) == 0
    for lo in range(0, flat.numel(), 16384):
        dist = (m[lo:lo + 16384, None] - mags[None, :]).abs()
        best = dist == dist.amin(dim=1, keepdim=True)            # one code, or two neighbours at a tie
        assert int(best.sum(1).max()) <= 2
        pick = torch.where(best.sum(1, keepdim=True) == 2, best & even[None, :], best)
        assert bool((pick.sum(1) == 1).all())
        out[lo:lo + 16384] = pick.float().argmax(1).to(u8)
    out |= (torch.signbit(flat) & ~nan).to(u8) << 7
    out[nan] = 0x7F
    return out.reshape(q.shape), nan.reshape(q.shape)


def same_bytes(got, want):
    """e4m3fn bytes equal, NaN codes compared by class"""
    g, w = got.cpu(), want.cpu()
    gn, wn = (g & 0x7F) == 0x7F, (w & 0x7F) == 0x7F
    return bool(torch.equal(gn, wn)) and bool(torch.equal(g[~wn], w[~wn]))


def same(got, want):
    """a cache against the reference's (either may be on the device): bits, NaN bytes of an fp8 cache by class"""
    return same_bytes(got, want) if want.dtype == u8 else torch.equal(got.cpu(), want.cpu())
