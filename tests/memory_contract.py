"""What tests/test_memory_contract.py shares (no tests in here): the calls of the library as `Call` objects -- the tensors a call takes
(`specs`, `data`), the C entry point on them (`run`), the outputs to compare (`outs`) and the exact workspace size -- and `place()`,
which lays a call's tensors out either the torch way or inside one guarded arena (tests/arena.py).

A call is run through the C ABI (`fa.lib()`), never a Python front, because the fronts allocate the LSE and the backward's workspace
themselves.  The split-KV family goes through its `_window` entry points, whose windowSize = 0 IS the sibling call.
"""
import ctypes
import math

import torch

import __graft_entry__ as entry

fa = entry.load_package()
import arena as ar  # noqa: E402
import kv_cache_check as kv  # noqa: E402
import kv_append_check as kvc  # noqa: E402
import weight_probe as wp  # noqa: E402
from abi_decl import c_call  # noqa: E402

DEV = "cuda:0"
bf, f32, u8, i32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32
F8 = kv.F8
CODE = {f32: fa.FA_DTYPE_F32, bf: fa.FA_DTYPE_BF16, F8: fa.FA_DTYPE_FP8_E4M3, torch.float16: fa.FA_DTYPE_F16}
PLACEMENTS = ("aligned", "offset")          # in this order: a failure under `aligned` is a workspace or guard finding, not an address one


class Call:
    def __init__(self, specs, data, run, outs, ws_bytes=0, note=""):
        self.specs, self.data, self.run, self.outs, self.ws_bytes, self.note = specs, data, run, outs, int(ws_bytes), note


def spec(shape, dtype, writable=False, side=False, strides=None):
    return dict(shape=tuple(shape), dtype=dtype, writable=writable, side=side, strides=strides)


def model_strides(H, S, d):
    """element strides of the [1, H, S, d] view of a (1, S, H * d) model-layout buffer"""
    return (S * H * d, d, H * d, 1)


def place(call, placement):
    """-> (arena or None, {name: device tensor}).  placement None: plain torch allocations, outputs and workspace zeroed (benign);
    "aligned": everything at 0 mod 512 inside one arena; "offset": 16 mod 256, side inputs 4 mod 16; ("only", name): `name` alone at
    its offset residue, the rest aligned.  In an arena the outputs and the workspace enter the call as 0xFF bytes (NaNs)."""
    specs = dict(call.specs)
    if call.ws_bytes and "ws" not in specs:
        specs["ws"] = spec((call.ws_bytes,), u8, writable=True)
    if placement is None:
        v = {}
        for n, s in specs.items():
            flat = torch.zeros(ar.extent(s["shape"], s["strides"]) * ar.itemsize(s["dtype"]), dtype=u8, device=DEV)
            flat = flat if s["dtype"] == u8 else flat.view(s["dtype"])
            v[n] = flat.view(s["shape"]) if s["strides"] is None else torch.as_strided(flat, s["shape"], s["strides"])
            if n in call.data:
                ar.bits(v[n]).copy_(ar.bits(call.data[n]))
        return None, v

    def residue(n, s):
        shifted = placement == "offset" or placement == ("only", n)
        return (ar.SIDE if s["side"] else ar.OFFSET) if shifted else ar.ALIGNED

    arena, v = ar.Arena.of(DEV, {n: dict(shape=s["shape"], dtype=s["dtype"], strides=s["strides"], writable=s["writable"],
                                          residue=residue(n, s)) for n, s in specs.items()})
    for n, t in call.data.items():
        arena.load(v[n], t)
    for n, s in specs.items():
        r, m = residue(n, s)
        assert v[n].data_ptr() % m == r, n
    return arena, v


def run(call, placement):
    arena, v = place(call, placement)
    call.run(v)
    torch.cuda.synchronize()
    return arena, v


def same(a, b):
    return torch.equal(ar.bits(a), ar.bits(b))


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def strides(*ts):
    keep = [fa.FaStrides(*t.stride()[:3]) for t in ts]
    return keep, [ctypes.byref(s) for s in keep]


def ptr(v, name):
    return v[name].data_ptr() if name in v else None


def randn(shape, seed, dtype=bf):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


# ---- forward ----------------------------------------------------------------------------------------------------------------------
def forward_call(c, p):
    """wp.FwdCase c with the inputs p = wp.build_forward(c): Q, K, V, O and (c.lse) the LSE through flash_attention_gqa"""
    dt = F8 if c.idt == "fp8" else c.idt
    st = (lambda H, S: model_strides(H, S, c.d)) if c.layout == "model" else (lambda H, S: None)
    specs = dict(Q=spec((1, c.H, c.Sq, c.d), dt, strides=st(c.H, c.Sq)), K=spec((1, c.Hkv, c.Sk, c.d), dt, strides=st(c.Hkv, c.Sk)),
                 V=spec((1, c.Hkv, c.Sk, c.d), dt, strides=st(c.Hkv, c.Sk)), O=spec((1, c.H, c.Sq, c.d), c.odt, True, strides=st(c.H, c.Sq)))
    if c.lse:
        specs["lse"] = spec((1, c.H, c.Sq), f32, True)
    idt, odt, flags = wp.forward_codes(c)

    def go(v):
        keep, refs = strides(v["Q"], v["K"], v["V"], v["O"])
        rc = fa.lib().flash_attention_gqa(v["Q"].data_ptr(), v["K"].data_ptr(), v["V"].data_ptr(), v["O"].data_ptr(), ptr(v, "lse"),
                                          1, c.H, c.Hkv, c.Sq, c.Sk, c.d, 1.0 / math.sqrt(c.d), c.causal, idt, odt, *refs, flags, stream())
        assert rc == 0, fa.error_string(rc)

    return Call(specs, {n: p[n] for n in ("Q", "K", "V")}, go, ["O"] + (["lse"] if c.lse else []))


def weights_call(Q, K, lse, causal):
    """flash_attention_weights on CPU tensors Q, K [B, H, S, d] and the LSE of a forward call"""
    B, H, Sq, d = Q.shape
    Sk = K.shape[2]
    specs = dict(Q=spec(Q.shape, Q.dtype), K=spec(K.shape, K.dtype), lse=spec(lse.shape, f32), P=spec((B, H, Sq, Sk), f32, True))

    def go(v):
        keep, refs = strides(v["Q"], v["K"])
        rc = fa.lib().flash_attention_weights(v["Q"].data_ptr(), v["K"].data_ptr(), v["lse"].data_ptr(), v["P"].data_ptr(), B, H, Sq, Sk, d,
                                              1.0 / math.sqrt(d), causal, CODE[Q.dtype], *refs, stream())
        assert rc == 0, fa.error_string(rc)

    return Call(specs, dict(Q=Q, K=K, lse=lse), go, ["P"])


# ---- backward ---------------------------------------------------------------------------------------------------------------------
def backward_call(Q, K, V, dO, causal, o_dtype, grad_dtype, layout="dense"):
    """flash_attention_backward_gqa on CPU tensors Q [B, H, Sq, d], K, V [B, Hkv, Sk, d] (bf16) and dO (o_dtype); O and the LSE come
    from the library's forward on plain allocations.  layout "model": all nine tensors as views of (B, S, heads * d) buffers (B = 1)"""
    B, H, Sq, d = Q.shape
    Hkv, Sk = K.shape[1:3]
    scale = 1.0 / math.sqrt(d)
    O, lse = fa.flash_attention(Q.to(DEV), K.to(DEV), V.to(DEV), is_causal=causal, out_dtype=o_dtype, return_lse=True)
    torch.cuda.synchronize()
    assert layout == "dense" or B == 1
    st = (lambda h, S: model_strides(h, S, d)) if layout == "model" else (lambda h, S: None)
    q, k = (lambda dt, w=False: spec((B, H, Sq, d), dt, w, strides=st(H, Sq))), (lambda dt, w=False: spec((B, Hkv, Sk, d), dt, w, strides=st(Hkv, Sk)))
    specs = dict(Q=q(bf), K=k(bf), V=k(bf), O=q(o_dtype), dO=q(o_dtype), lse=spec((B, H, Sq), f32),
                 dQ=q(grad_dtype, True), dK=k(grad_dtype, True), dV=k(grad_dtype, True))

    def go(v):
        keep, refs = strides(*(v[n] for n in ("Q", "K", "V", "O", "dO", "dQ", "dK", "dV")))
        rc = fa.lib().flash_attention_backward_gqa(*(v[n].data_ptr() for n in ("Q", "K", "V", "O", "dO", "lse", "dQ", "dK", "dV", "ws")),
                                                   B, H, Hkv, Sq, Sk, d, scale, causal, fa.FA_DTYPE_BF16, CODE[o_dtype], CODE[grad_dtype],
                                                   *refs, stream())
        assert rc == 0, fa.error_string(rc)

    return Call(specs, dict(Q=Q, K=K, V=V, O=O.cpu(), dO=dO.to(o_dtype), lse=lse.cpu()), go, ["dQ", "dK", "dV"],
                fa.backward_workspace_size(B, H, Sq, d))


# ---- the split-KV family ----------------------------------------------------------------------------------------------------------
HKV, G, CAPACITY = 2, 4, 384
FORMS = [(page, fp8) for fp8 in (False, True) for page in (None, 16, 128)]
WIDE = 3                                                      # the page-16 table is a row slice of one this much wider
PLANS = {"decode": fa.decode_plan, "extend": fa.extend_plan, "varlen": fa.extend_varlen_plan}


class Cache:
    """a K/V cache of `B` sequences in one of the forms: the CPU tensors a call takes (K, V: the cache or the pools; table; kd, vd),
    and the float64 logical cache refK, refV [B, Hkv, CAPACITY, d] the references read"""

    def __init__(self, B, d, page, fp8, seed):
        K, V = randn((B, HKV, CAPACITY, d), seed), randn((B, HKV, CAPACITY, d), seed + 1)
        self.B, self.d, self.page, self.fp8, self.kd, self.vd, self.table = B, d, page, fp8, None, None, None
        if fp8:
            (K, self.kd), (V, self.vd) = kv.quantise(K.float() * 3.0), kv.quantise(V.float() * 0.5)      # uint8; descales away from 1
            self.refK, self.refV = kv.dequantise(K, self.kd), kv.dequantise(V, self.vd)
        else:
            self.refK, self.refV = K.double(), V.double()
        if page:
            n = CAPACITY // page
            table = kv.random_table(B, n, seed + 2)
            pools = kv.scatter(K, table, page), kv.scatter(V, table, page)
            assert torch.equal(kv.gather(pools[0], table), K) and torch.equal(kv.gather(pools[1], table), V)
            K, V = pools
            self.table = torch.cat([table, torch.full((B, WIDE), 2 ** 31 - 1, dtype=i32)], 1) if page == 16 else table
        self.K, self.V = (t.view(F8) if fp8 else t for t in (K, V))

    def specs(self, writable=False):
        s = dict(K=spec(self.K.shape, self.K.dtype, writable), V=spec(self.V.shape, self.V.dtype, writable))
        if self.page:
            s["table"] = spec(self.table.shape, i32, side=True)
        if self.fp8:
            s["kd"], s["vd"] = spec((HKV,), f32, side=True), spec((HKV,), f32, side=True)
        return s

    def data(self):
        d = dict(K=self.K, V=self.V)
        if self.page:
            d["table"] = self.table
        if self.fp8:
            d["kd"], d["vd"] = self.kd, self.vd
        return d

    def values(self, v):
        """what a call on the placed tensors `v` takes from the cache, by abi_decl's names: K, V and their strides, the lengths,
        cuSeqlensQ of a ragged call, the descales, the cache's type, and the capacity or the table and the paging geometry"""
        _, (sK, sV) = strides(v["K"], v["V"])                   # (a byref holds on to its fa_strides)
        out = dict(K=v["K"].data_ptr(), V=v["V"].data_ptr(), sK=sK, sV=sV, lens=v["lens"].data_ptr(), cu=ptr(v, "cu"), kd=ptr(v, "kd"),
                   vd=ptr(v, "vd"), kv=CODE[self.K.dtype], B=self.B, Hkv=HKV, d=self.d)
        if not self.page:
            return dict(out, Sk=CAPACITY)
        return dict(out, table=v["table"].data_ptr(), P=self.K.shape[0], page=self.page, maxp=CAPACITY // self.page, ts=self.table.shape[1])


def split_kv_call(family, cache, Q, lens, causal, ns, W, cu=None, odt=f32, sink=False):
    """decode / extend: Q [B, H, Sq, d]; varlen: Q [T, H, d] packed by token with cu (B + 1 ints).  O in `odt`, the LSE fp32.  The plan is
    asserted: the forced split count is taken, and the combine kernel runs exactly when there is more than one split.  sink: through
    the family's flash_attention_sink_* entry point, on the tensor `sinks` that the caller adds to specs and data"""
    d, H, B = cache.d, HKV * G, cache.B
    ragged = family == "varlen"
    rows = Q.shape[0] if ragged else Q.shape[2]
    plan = PLANS[family](B, H, HKV, rows, CAPACITY, d, CODE[odt], ns, window=W)
    assert plan["num_splits"] == ns and plan["kv_block_rows"] == 128 and (plan["combine_grid"] > 0) == (ns > 1), plan
    specs = dict(cache.specs(), Q=spec(Q.shape, bf), O=spec(Q.shape, odt, True), lse=spec((H, rows) if ragged else (B, H, rows), f32, True),
                 lens=spec((B,), i32, side=True))
    data = dict(cache.data(), Q=Q, lens=torch.tensor(lens, dtype=i32))
    if ragged:
        specs["cu"], data["cu"] = spec((B + 1,), i32, side=True), torch.tensor(cu, dtype=i32)
    name = ("decode" if family == "decode" else "extend") + ("_paged" if cache.page else "") + ("_varlen" if ragged else "")
    name = "flash_attention_" + ("sink_" + name if sink else name + "_window")

    def go(v):
        _, (sQ, sO) = (None, (None, None)) if ragged else strides(v["Q"], v["O"])    # NULL: the token-major [T, H, d] an engine holds
        values = dict(cache.values(v), Q=v["Q"].data_ptr(), O=v["O"].data_ptr(), LSE=v["lse"].data_ptr(), ws=ptr(v, "ws"), H=H, Sq=rows,
                      scale=1.0 / math.sqrt(d), causal=causal, dtype=fa.FA_DTYPE_BF16, o=CODE[odt], ns=ns, W=W, sQ=sQ, sO=sO, stream=stream())
        if sink:
            values["sinks"] = v["sinks"].data_ptr()
        rc = c_call(name, values)
        assert rc == 0, (name, fa.error_string(rc))

    return Call(specs, data, go, ["O", "lse"], fa.decode_workspace_size(1 if ragged else B, H, rows, d, ns),
                f"{name} d {d} rows {rows} causal {causal} splits {ns} window {W} O {odt}")


# ---- cache append -----------------------------------------------------------------------------------------------------------------
def append_call(cache, Knew, Vnew, lens, cu=None):
    """kv_append into `cache` (whose K, V are then writable): Knew, Vnew [B, Hkv, Sq, d], or with cu [T, Hkv, d] packed by token"""
    ragged = cu is not None
    rows = Knew.shape[0] if ragged else Knew.shape[2]
    specs = dict(cache.specs(writable=True), Knew=spec(Knew.shape, bf), Vnew=spec(Vnew.shape, bf), lens=spec((cache.B,), i32, side=True))
    data = dict(cache.data(), Knew=Knew, Vnew=Vnew, lens=torch.tensor(lens, dtype=i32))
    if ragged:
        specs["cu"], data["cu"] = spec((cache.B + 1,), i32, side=True), torch.tensor(cu, dtype=i32)
    name = "flash_attention_kv_append" + ("_paged" if cache.page else "") + ("_varlen" if ragged else "")

    def go(v):
        _, (sKn, sVn) = (None, (None, None)) if ragged else strides(v["Knew"], v["Vnew"])
        rc = c_call(name, dict(cache.values(v), Kn=v["Knew"].data_ptr(), Vn=v["Vnew"].data_ptr(), Sq=rows, dtype=fa.FA_DTYPE_BF16,
                               sKn=sKn, sVn=sVn, stream=stream()))
        assert rc == 0, (name, fa.error_string(rc))

    return Call(specs, data, go, ["K", "V"], 0, name)


def appended(cache, which, new, lens, cu=None):
    """kv_append_check.append's bytes of the cache K or V (`which`) after the call, sequence by sequence for a ragged one"""
    stored = getattr(cache, which)
    ints = stored.view(u8) if cache.fp8 else stored.view(torch.int16)
    ds = getattr(cache, "kd" if which == "K" else "vd")
    table = cache.table[:, :CAPACITY // cache.page] if cache.page else None
    if cu is None:
        return kvc.append(new, ints, lens, ds, table)
    out = ints.clone()
    for b in range(cache.B):
        if cu[b + 1] == cu[b]:
            continue
        one = new[cu[b]:cu[b + 1]].transpose(0, 1)[None].contiguous()
        if table is None:
            out[b:b + 1] = kvc.append(one, out[b:b + 1], [lens[b]], ds)
        else:
            out = kvc.append(one, out, [lens[b]], ds, table[b:b + 1])
    return out
