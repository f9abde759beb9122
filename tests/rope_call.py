"""What the tests of flash_attention_rope_append* share besides the reference (tests/rope_check.py; no tests in here): the calls BY
NAME from include/flash_attention.h, as tests/abi_decl.py makes them, with the short keys of the arguments these entry points add.

* `c_call(symbol, values)`: abi_decl.c_call over `KEYS` = abi_decl's and Qo / cs / rot / maxpos / il / sQo.
* `host_calls(...)`: abi_decl.host_calls for these entry points -- every tensor and the table on one aligned HOST pointer, six strides.
* `launch(...)`: a call on device tensors -- the form (contiguous / paged, uniform / ragged) from which arguments are given, the
  strides from the tensors, the cache type from the caches' integer dtype (int16: bf16 patterns, uint8: e4m3fn bytes).
* `twin(...)`: flash_attention_kv_append* of the same form on the same caches, by name through abi_decl.c_call.
"""
import ctypes

import torch

import abi_decl
from abi_decl import BF16, FP8, fa

KEYS = dict(abi_decl.KEYS, Qo=("Qout",), cs=("cosSin",), rot=("rotDim",), maxpos=("maxPos",), il=("interleaved",), sQo=("sQout",))
STRIDES = ("sQ", "sKnew", "sVnew", "sQout", "sK", "sV")          # in declared order
ROPE = {(False, False): "flash_attention_rope_append", (True, False): "flash_attention_rope_append_paged",
        (False, True): "flash_attention_rope_append_varlen", (True, True): "flash_attention_rope_append_paged_varlen"}
TWIN = {k: v.replace("rope_append", "kv_append") for k, v in ROPE.items()}


def c_call(symbol, values):
    """abi_decl.c_call with the keys above: every declared parameter is looked up under its short key, none may be missing or given
    twice; `strides` = the six fa_strides* together, in declared order"""
    values = dict(values)
    together = values.pop("strides", None)
    unknown = set(values) - set(KEYS)
    assert not unknown, (symbol, sorted(unknown))
    params = abi_decl.declared_parameters(symbol)
    found = {}
    if together is not None:
        names = [n for n in params if n in STRIDES]
        assert len(names) == len(together), (symbol, names)
        found = {n: [s] for n, s in zip(names, together)}
    for key, value in values.items():
        for n in KEYS[key]:
            if n in params:
                found.setdefault(n, []).append(value)
    args = []
    for n in params:
        if len(found.get(n, ())) != 1:
            raise KeyError(f"{symbol}: {len(found.get(n, ()))} values for the declared parameter {n}")
        args.append(found[n][0])
    return getattr(fa.lib(), symbol)(*args)


def host_calls(*symbols_and_oks):
    """(symbol, ok), ... -> (call, ..., p): call(**overrides) is `symbol` with every tensor, cuSeqlensQ, the block table and the
    cos / sin table at the aligned host pointer p, no lengths, descales, strides or stream, and the ints of `ok`"""
    buf, p = abi_decl.aligned_host_pointer()

    def make(symbol, ok):
        base = dict(dict(Q=p, Kn=p, Vn=p, Qo=p, K=p, V=p, cs=p, cu=p, table=p, lens=None, kd=None, vd=None, strides=[None] * 6, stream=None), **ok)

        def call(_keep=buf, **overrides):
            return c_call(symbol, dict(base, **overrides))

        return call

    return (*(make(s, ok) for s, ok in symbols_and_oks), p)


def strides3(t, ragged=False):
    """fa_strides of a [B, heads, rows, d] view, or of a token-packed [T, heads, d] one"""
    assert t.stride(-1) == 1
    return fa.FaStrides(0, t.stride(1), t.stride(0)) if ragged else fa.FaStrides(*t.stride()[:3])


def _geometry(K, block_table):
    if block_table is None:
        return dict(Sk=K.shape[2])
    assert block_table.dtype == torch.int32 and block_table.stride(1) == 1
    return dict(table=block_table.data_ptr(), P=K.shape[0], page=K.shape[2], maxp=block_table.shape[1],
                ts=block_table.stride(0) if block_table.shape[0] > 1 else block_table.shape[1])


def _ptr(t):
    return None if t is None else t.data_ptr()


def launch(Q, Kn, Vn, Qo, K, V, cs, lens=None, il=False, kd=None, vd=None, block_table=None, cu=None, B=None, stream=None,
           check=True):
    """flash_attention_rope_append* on device tensors; ragged (cu given): Q / Qo [T, H, d], Kn / Vn [T, Hkv, d], B = len(cu) - 1"""
    ragged = cu is not None
    assert K.dtype in (torch.int16, torch.uint8) and V.dtype == K.dtype and cs.dtype == torch.float32 and cs.is_contiguous()
    keep = [strides3(Q, ragged), strides3(Kn, ragged), strides3(Vn, ragged), strides3(Qo, ragged), strides3(K), strides3(V)]
    values = dict(Q=Q.data_ptr(), Kn=Kn.data_ptr(), Vn=Vn.data_ptr(), Qo=Qo.data_ptr(), K=K.data_ptr(), V=V.data_ptr(), cs=cs.data_ptr(),
                  lens=_ptr(lens), kd=_ptr(kd), vd=_ptr(vd), B=(cu.numel() - 1 if ragged else Q.shape[0]) if B is None else B,
                  H=Q.shape[1], Hkv=Kn.shape[1], Sq=Q.shape[0] if ragged else Q.shape[2], d=Q.shape[-1], rot=cs.shape[1],
                  maxpos=cs.shape[0], il=int(il), dtype=BF16, kv=FP8 if K.dtype == torch.uint8 else BF16,
                  strides=[ctypes.byref(s) for s in keep], stream=None if stream is None else ctypes.c_void_p(stream.cuda_stream),
                  **_geometry(K, block_table))
    if ragged:
        values["cu"] = cu.data_ptr()
    if stream is None:
        values["stream"] = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = c_call(ROPE[block_table is not None, ragged], values)
    if check:
        assert rc == 0, (rc, fa.error_string(rc))
    return rc


def twin(Kn, Vn, K, V, lens=None, kd=None, vd=None, block_table=None, cu=None):
    """flash_attention_kv_append* of the same form on the same kinds of tensors"""
    ragged = cu is not None
    keep = [strides3(Kn, ragged), strides3(Vn, ragged), strides3(K), strides3(V)]
    values = dict(Kn=Kn.data_ptr(), Vn=Vn.data_ptr(), K=K.data_ptr(), V=V.data_ptr(), lens=_ptr(lens), kd=_ptr(kd), vd=_ptr(vd),
                  B=cu.numel() - 1 if ragged else Kn.shape[0], Hkv=Kn.shape[1], Sq=Kn.shape[0] if ragged else Kn.shape[2], d=Kn.shape[-1],
                  dtype=BF16, kv=FP8 if K.dtype == torch.uint8 else BF16, strides=[ctypes.byref(s) for s in keep],
                  stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), **_geometry(K, block_table))
    if ragged:
        values["cu"] = cu.data_ptr()
    rc = abi_decl.c_call(TWIN[block_table is not None, ragged], values)
    assert rc == 0, (rc, fa.error_string(rc))
