"""Checker shared by the split-KV decode tests (tests/test_decode.py, test_decode_paged.py, test_decode_fp8.py, test_decode_edges.py,
weight_probe.py): the project's float64 ground truth for decode, the element-wise criterion, and the data the tests build alike.
Plain torch on the CPU for everything but `assert_close`, which takes device results.

Reference.  `reference()`: the explicit softmax in float64 over the keys each sequence can see (`visible()`: the bottom-right
aligned mask), grouped-query attention by `repeat_interleave` of the K/V heads.  K and V may be bf16, fp32 or float64 -- an fp8 cache
comes in dequantised (`dequantise()`: exact in float64), so the error of quantising is never part of a comparison.

Criterion.  `assert_close()`: every element of O within the project's stated 1e-3 + 1e-3 |ref|, every LSE within 2e-4 + 2e-6 |ref|,
both finite.  It prints the worst ratio of each (and the worst absolute LSE error, the figure the logs under profiles/ carry).
"""
import torch

import __graft_entry__ as entry

fa = entry.load_package()

DEV = "cuda:0"
CAP = fa.FA_DECODE_MAX_SPLITS
TILE = 128   # fa_decode_plan.kv_block_rows
F8 = getattr(torch, "float8_e4m3fn", None)   # (the bf16 tests do not need it)


def randn(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


def visible(L, Sq, causal):
    """bool [Sq, L]: row i sees key k.  Bottom-right aligned: the Sq rows are the last rows of the L keys; at least key 0"""
    k = torch.arange(L)[None, :]
    if not causal:
        return torch.ones(Sq, L, dtype=torch.bool) & (k >= 0)
    last = (L - Sq + torch.arange(Sq)).clamp(min=0)[:, None]
    return k <= last


def reference(Q, K, V, lens, causal, scale=None):
    """float64 explicit softmax over the visible keys of each sequence (CPU tensors; K, V [B, Hkv, capacity, d] in bf16, fp32 or
    float64: a paged cache gathered, an fp8 one dequantised): O [B, H, Sq, d], LSE [B, H, Sq]"""
    B, H, Sq, d = Q.shape
    G = H // K.shape[1]
    scale = scale or 1.0 / d ** 0.5
    O = torch.zeros(B, H, Sq, d, dtype=torch.float64)
    lse = torch.zeros(B, H, Sq, dtype=torch.float64)
    for b in range(B):
        L = K.shape[2] if lens is None else int(lens[b])
        k = K[b, :, :L].double().repeat_interleave(G, 0)
        v = V[b, :, :L].double().repeat_interleave(G, 0)
        S = (Q[b].double() @ k.transpose(-1, -2)) * scale
        S = S.masked_fill(~visible(L, Sq, causal)[None], float("-inf"))
        lse[b] = torch.logsumexp(S, -1)
        O[b] = torch.softmax(S, -1) @ v
    return O, lse


def assert_close(O, lse, refO, refL, what=""):
    O, lse = O.double().cpu(), lse.double().cpu()
    assert torch.isfinite(O).all() and torch.isfinite(lse).all(), what
    err, tol = (O - refO).abs(), 1e-3 + 1e-3 * refO.abs()
    lerr, ltol = (lse - refL).abs(), 2e-4 + 2e-6 * refL.abs()
    print(f"{what}: worst O error / tolerance {(err / tol).max().item():.3f}, worst LSE error / tolerance {(lerr / ltol).max().item():.3f}"
          f" ({lerr.max().item():.2e})")
    assert (err <= tol).all(), f"{what}: {int((err > tol).sum())} elements outside 1e-3 + 1e-3|ref|, worst ratio {(err / tol).max().item():.3f}"
    assert (lerr <= ltol).all(), f"{what}: LSE error {lerr.max().item():.3e}"


# ---- paged caches ----
def gather(pool, table):
    """[P, Hkv, page, d] pool, [B, max_pages] table (in range) -> the contiguous cache [B, Hkv, max_pages * page, d]"""
    B, n = table.shape
    P, Hkv, page, d = pool.shape
    return pool[table.long()].permute(0, 2, 1, 3, 4).reshape(B, Hkv, n * page, d).contiguous()


def boundary_lengths(page, cap):
    """around every boundary: the page, the 128-key tile, the capacity"""
    return sorted({max(1, min(L, cap)) for L in (1, page - 1, page, page + 1, 127, 128, 129, cap - 3, cap)})


def max_pages_of(page):
    return max(3, 320 // page)     # capacities 320, 320, 384, 768: more than one tile, more than two pages


def paged_layout(page, d, spare=7):
    """(P, table, lens) of the paged sweeps: one sequence per boundary length, pools of P pages -- `spare` more than the sequences
    use -- and a random permutation as the table.  The pools are randn((P, Hkv, page, d), 1000 / 2000 + page + d) in the caller's type"""
    n = max_pages_of(page)
    lens = boundary_lengths(page, n * page)
    B = len(lens)
    P = B * n + spare
    g = torch.Generator().manual_seed(3000 + page + d)
    table = torch.randperm(P, generator=g)[:B * n].reshape(B, n).to(torch.int32)
    return P, table, lens


# ---- fp8 caches, handled as uint8 tensors and viewed as float8_e4m3fn at the call ----
def quantise(x):
    """x fp32 [*, Hkv, rows, d] (K/V heads in dimension 1) -> (bytes uint8 of the same shape, descale fp32 [Hkv] = amax / 448).
    torch's cast gives NaN beyond 448, not saturation: clamp, and check"""
    ds = (x.abs().amax(dim=(0, 2, 3)) / 448.0).float()
    b = (x / ds[None, :, None, None]).clamp(-448, 448).to(F8).view(torch.uint8)
    assert ((b & 0x7F) != 0x7F).all(), "NaN among the quantised bytes"
    return b, ds


def dequantise(b, ds):
    return b.view(F8).float().double() * ds.double()[None, :, None, None]
