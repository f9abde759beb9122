"""Checker of the shared-prefix (cascade) decode tests: the float64 ground truth, the data in the four cache forms and the fronts.

Rule.  The logical cache of sequence b is [shared[0 : ls) ; unique_b[0 : len_b)], ls and len_b clamped into [1, capacity] as the
library clamps them.  Every one of the Sq rows sees ALL ls shared keys; of its own suffix it sees `kv_cache_check.visible(len_b, Sq,
causal)` -- what flash_attention_decode shows it on the suffix alone, "at least key 0" included.

Reference.  `reference()` is `kv_cache_check.reference` on the concatenated caches with `vis=` built from that rule, float64 on the
CPU; fp8 caches come in dequantised.  Criterion: `kv_cache_check.assert_close`, unchanged.
"""
import torch

import kv_cache_check as kc
from kv_cache_check import DEV, F8, fa

LS_CAP, LU_CAP = 384, 256      # the capacities of the shared part and of the suffixes in every GPU case


def clamp(n, cap):
    return min(max(int(n), 1), cap)


def concatenated(Ks, Vs, K, V, ls, lens):
    """(Kc, Vc [B, Hkv, ls + capacity, d], lens_c): sequence b's logical cache, its suffix directly behind the ls shared keys"""
    B = K.shape[0]
    ls = clamp(ls, Ks.shape[1])
    lens = [clamp(K.shape[2] if lens is None else lens[b], K.shape[2]) for b in range(B)]
    Kc = torch.cat([Ks[None, :, :ls].expand(B, -1, -1, -1).double(), K.double()], 2)
    Vc = torch.cat([Vs[None, :, :ls].expand(B, -1, -1, -1).double(), V.double()], 2)
    return Kc, Vc, [ls + L for L in lens]


def visibility(ls, lens, Sq, causal):
    """vis(b, h, L) of kv_cache_check.reference: the shared part fully visible, the rule of decode on the suffix"""
    def vis(b, h, L):
        assert L == ls + lens[b]
        return torch.cat([torch.ones(Sq, ls, dtype=torch.bool), kc.visible(lens[b], Sq, causal)], 1)
    return vis


def reference(Q, Ks, Vs, K, V, ls, lens, causal, sinks=None, scale=None):
    """float64 (O [B, H, Sq, d], LSE [B, H, Sq]) of the cascade call; Ks, Vs [Hkv, capacity, d], K, V [B, Hkv, capacity, d] (CPU;
    bf16, fp32 or float64: a paged cache gathered, an fp8 one dequantised)"""
    Kc, Vc, lens_c = concatenated(Ks, Vs, K, V, ls, lens)
    ls = clamp(ls, Ks.shape[1])
    return kc.reference(Q, Kc, Vc, lens_c, causal, sinks=sinks, vis=visibility(ls, [L - ls for L in lens_c], Q.shape[2], causal),
                        scale=scale)


class Caches:
    """The two caches of a cascade call, N(0, 1) data, in one of the four forms.  sK, sV [Hkv, LS_CAP, d] and uK, uV [B, Hkv, LU_CAP, d]:
    what is stored, contiguous, on the CPU (bf16, or the e4m3fn bytes as uint8 with ONE descale pair kd, vd for both parts); ref*: the
    float64 logical caches.  page: 0, or the page size of the one pool that holds both parts (shared_table [LS_CAP / page], block_table
    [B, LU_CAP / page], a random permutation with spare pages)"""

    def __init__(self, B, Hkv, d, page, fp8, seed, sK=None, sV=None, uK=None, uV=None):
        g, bf16 = torch.Generator().manual_seed(seed), torch.bfloat16
        mk = lambda t, shape: torch.randn(shape, generator=g).to(bf16) if t is None else t
        sK, sV = mk(sK, (Hkv, LS_CAP, d)), mk(sV, (Hkv, LS_CAP, d))
        uK, uV = mk(uK, (B, Hkv, LU_CAP, d)), mk(uV, (B, Hkv, LU_CAP, d))
        self.B, self.Hkv, self.d, self.page, self.fp8, self.kd, self.vd = B, Hkv, d, page, fp8, None, None
        if fp8:
            def q(s, u):      # one descale per K/V head over both parts; saturation cannot happen: amax / 448
                ds = (torch.maximum(s.float().abs().amax(dim=(1, 2)), u.float().abs().amax(dim=(0, 2, 3))) / 448.0).float()
                to8 = lambda x, dim: (x.float() / ds.view([-1 if i == dim else 1 for i in range(x.dim())])).to(F8).view(torch.uint8)
                return to8(s, 0), to8(u, 1), ds
            self.sK, self.uK, self.kd = q(sK, uK)
            self.sV, self.uV, self.vd = q(sV, uV)
            deq = lambda b8, ds, dim: b8.view(F8).float().double() * ds.double().view([-1 if i == dim else 1 for i in range(b8.dim())])
            self.refsK, self.refuK = deq(self.sK, self.kd, 0), deq(self.uK, self.kd, 1)
            self.refsV, self.refuV = deq(self.sV, self.vd, 0), deq(self.uV, self.vd, 1)
        else:
            self.sK, self.sV, self.uK, self.uV = sK, sV, uK, uV
            self.refsK, self.refsV, self.refuK, self.refuV = sK.double(), sV.double(), uK.double(), uV.double()
        if page:
            ns, nu = LS_CAP // page, LU_CAP // page
            self.spare = 5
            perm = torch.randperm(ns + B * nu + self.spare, generator=torch.Generator().manual_seed(seed + 2)).to(torch.int32)
            self.shared_table, self.block_table = perm[:ns].clone(), perm[ns:ns + B * nu].reshape(B, nu).clone()
            self.unused = perm[ns + B * nu:]

    def pool(self, s, u, fill=0):
        """the pool [P, Hkv, page, d] that holds s under shared_table and u under block_table; the spare pages hold `fill` bytes"""
        page, Hkv, d = self.page, self.Hkv, self.d
        P = self.shared_table.numel() + self.block_table.numel() + self.spare
        pool = torch.zeros((P, Hkv, page, d), dtype=s.dtype)
        pool.view(torch.uint8).fill_(fill)
        pool[self.shared_table.long()] = s.reshape(Hkv, -1, page, d).transpose(0, 1)
        pool[self.block_table.long().reshape(-1)] = u.reshape(self.B, Hkv, -1, page, d).permute(0, 2, 1, 3, 4).reshape(-1, Hkv, page, d)
        return pool

    def device(self, sK=None, sV=None, uK=None, uV=None, contiguous=False, fill=0, shared_table=None, block_table=None):
        """the positional cache arguments of the front and the descales as keywords, of the stored bytes (or of the given ones in
        their place: a poisoned copy).  contiguous: the contiguous form of the same bytes, whatever the page"""
        t = [self.sK if sK is None else sK, self.sV if sV is None else sV, self.uK if uK is None else uK, self.uV if uV is None else uV]
        view = lambda x: (x.view(F8) if self.fp8 else x).to(DEV)
        ds = dict(k_descale=self.kd.to(DEV), v_descale=self.vd.to(DEV)) if self.fp8 else {}
        if self.page and not contiguous:
            st = self.shared_table if shared_table is None else shared_table
            bt = self.block_table if block_table is None else block_table
            return [view(self.pool(t[0], t[2], fill)), view(self.pool(t[1], t[3], fill)), st.to(DEV), bt.to(DEV)], ds
        return [view(x) for x in t], ds

    def reference(self, Q, ls, lens, causal, sinks=None):
        return reference(Q, self.refsK, self.refsV, self.refuK, self.refuV, ls, lens, causal, sinks=sinks)


def attend(args, ds, Q, ls, lens, **kw):
    """(O, LSE) -- or O alone under return_lse=False -- of one cascade call through the Python fronts; args, ds: Caches.device()"""
    front = fa.flash_attention_cascade_decode_paged if len(args) == 4 and args[2].dtype == torch.int32 else fa.flash_attention_cascade_decode
    kw.setdefault("return_lse", True)
    return front(Q, *args, None if ls is None else kc.i32([ls]), kc.i32(lens), **ds, **kw)
