"""Kit of the sparse MLA decode tests (flash_attention_mla_sparse_decode*), on mla_check's data, pools and tables
and kv_cache_check's criterion: the float64 reference, index lists with every kind of slot, the four cache forms behind one `attend`,
and a by-name caller of the C entry points.

Rule.  Slot t of query row (b, i) names position p = indices[b, i, t]; it is a key iff 0 <= p < lim, lim = len_b (clamped into
[1, capacity]) or, causal, max(len_b - Sq + i + 1, 1).  A position in two slots is two keys.  A row without a key: O = 0, LSE = -inf."""
import torch

import kv_cache_check as kc
import mla_check as mc
from abi_decl import declared_parameters
from kv_cache_check import DEV, fa

FORMS = [(fp8, page) for fp8 in (False, True) for page in (0,) + mc.PAGES]


def limit(L, Sq, i, causal):
    L = mc.clamp(L)
    return max(L - Sq + i + 1, 1) if causal else L


def reference(Q, KV, idx, lens, causal, scale=mc.DEFAULT_SCALE):
    """float64 (O [B, H, Sq, 512], LSE [B, H, Sq]): the row's valid slots gathered explicitly, a softmax over them, the first 512 columns
    of the same rows.  KV is the LOGICAL cache (an fp8 one dequantised)"""
    B, H, Sq, _ = Q.shape
    O = torch.zeros(B, H, Sq, mc.DL, dtype=torch.float64)
    lse = torch.full((B, H, Sq), float("-inf"), dtype=torch.float64)
    for b in range(B):
        for i in range(Sq):
            p = idx[b, i].long()
            kv = KV[b, p[(p >= 0) & (p < limit(lens[b], Sq, i, causal))]].double()
            if len(kv):
                S = (Q[b, :, i].double() @ kv.T) * scale
                lse[b, :, i] = torch.logsumexp(S, -1)
                O[b, :, i] = torch.softmax(S, -1) @ kv[:, :mc.DL]
    return O, lse


def assert_close(O, lse, refO, refL, what):
    """kv_cache_check.assert_close on the rows with a key; exactly O = 0 and LSE = -inf on the others"""
    O, lse = O.cpu(), lse.cpu()
    none = refL == float("-inf")
    assert (O[none] == 0).all() and (lse[none] == float("-inf")).all(), f"{what}: a row without a key"
    kc.assert_close(O, lse.masked_fill(none, 0.0), refO, refL.masked_fill(none, 0.0), what)


def index_lists(Sq, topk, lens, seed, batch=mc.B):
    """int32 [B, Sq, topk]: unsorted samples, half of them of [0, len_b) and half of [0, capacity) -- so positions at and beyond the
    length and positions the causal mask hides are among them -- with a duplicate, -1 scattered and trailing, the second tile of 32
    slots without a key (between tiles that have some), and row (1, 0) without any key"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, mc.CAPACITY, (batch, Sq, topk), generator=g, dtype=torch.int32)
    for b in range(batch):
        below = torch.randint(0, mc.clamp(lens[b]), (Sq, topk), generator=g, dtype=torch.int32)
        idx[b] = torch.where(torch.rand((Sq, topk), generator=g) < 0.5, below, idx[b])
    if topk > 1:
        idx[:, :, 1] = idx[:, :, 0]
    idx[torch.rand(idx.shape, generator=g) < 0.15] = -1
    idx[:, :, topk - topk // 8:] = -1
    for b in range(batch):
        beyond = mc.clamp(lens[b])                    # the first position that is no key of any row (the capacity: out of range)
        idx[b, :, 32:64:2] = beyond if beyond < mc.CAPACITY else -1
        idx[b, :, 33:64:2] = -1
    idx[1, 0] = -1
    idx[1, 0, ::3] = mc.clamp(lens[1]) if mc.clamp(lens[1]) < mc.CAPACITY else -1
    return idx


class Cache:
    """one latent cache in a form (fp8, page): `stored` [B, CAPACITY, 576] (bf16, or uint8 bytes of e4m3fn), the descale, the float64
    `logical` cache the reference reads, and for a paged form the table and the pool"""

    def __init__(self, KV, fp8, page, seed=77):
        self.fp8, self.page, self.ds = fp8, page, None
        self.stored, self.logical = KV, KV.double()
        if fp8:
            b, self.ds = kc.quantise(KV.float()[:, None])
            self.stored, self.logical = b[:, 0].contiguous(), kc.dequantise(b, self.ds)[:, 0]
        self.table = mc.table_for(KV.shape[0], page, seed) if page else None
        self.pool = mc.pool_of(self.stored, self.table, page) if page else None


def attend(Q, c, idx, lens, stored=None, table=None, pool=None, **kw):
    """(O, LSE) -- O alone under return_lse=False -- of the sparse call on Cache c; stored / table / pool replace the cache's own"""
    kw.setdefault("return_lse", True)
    dev = lambda t: (t.view(kc.F8) if c.fp8 else t).to(DEV)
    if c.fp8:
        kw["kv_descale"] = c.ds.reshape(1).to(DEV)
    if not c.page:
        return fa.flash_attention_mla_sparse_decode(Q.to(DEV), dev(c.stored if stored is None else stored), idx.to(DEV), kc.i32(lens), **kw)
    return fa.flash_attention_mla_sparse_decode_paged(Q.to(DEV), dev(c.pool if pool is None else pool),
                                                      (c.table if table is None else table).to(DEV), idx.to(DEV), kc.i32(lens), **kw)


def symbol(fp8, paged):
    return fa._MLA_SPARSE_SYMBOLS[bool(fp8)][bool(paged)]


def c_call(name, **named):
    """`name` on the arguments given under the header's own parameter names; names the symbol does not declare are ignored"""
    return getattr(fa.lib(), name)(*[named[n] for n in declared_parameters(name)])
