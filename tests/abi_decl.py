"""What the tests of the C ABI share (no tests in here): include/flash_attention.h as the one source of every argument list.

* `declared_parameters(symbol)`: the parameter names the header declares; `FA_ERR` and the code constants: its enums.
* `c_call(symbol, values)`: a call into the library BY NAME -- the positional list is built from the header, each parameter looked up
  in `values` under the short keys of `KEYS`.  No test writes the 20 to 33 positional arguments of a K/V-cache entry point by hand.
* `host_call(symbol, ok)`: `call(**overrides)` on aligned HOST memory, so that a call stops at the argument under test and no GPU is
  touched.  The refusal ladders of the callers stay theirs: a call that passes every check would launch on host pointers.
* `plan_call`, `tiles`, `MetaTensor`: the plan functions by name, the key tiles of a length, a tensor's metadata for the binding's checks.

Users: the CPU tests of the K/V-cache calls (test_decode_abi, test_decode_paged_abi, test_decode_fp8_abi, test_decode_window_abi,
test_extend_abi, test_extend_window_abi, test_extend_varlen_abi, test_kv_append_abi, test_rope_append_abi, test_sink_abi), the
device-pointer calls of the GPU tests (memory_contract.py and with it test_memory_contract / test_sink_memory_contract,
test_extend_varlen.py, rope_call.py and with it test_rope_append* / test_rope_memory_contract), and -- for the
constants and the host pointer -- test_gqa_abi and test_backward_abi."""
import ctypes
import functools
import os
import re

import __graft_entry__ as entry

fa = entry.load_package()


@functools.lru_cache(maxsize=None)
def _header():
    """include/flash_attention.h without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(entry.ROOT, "include", "flash_attention.h")).read(), flags=re.S)


@functools.lru_cache(maxsize=None)
def _declared(name):
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\((.*?)\)\s*;", _header(), flags=re.S)
    assert m, name
    return tuple(re.sub(r"[\s*]+", " ", a).split()[-1] for a in m.group(1).split(","))


def declared_parameters(name):
    """the parameter names of `name` as include/flash_attention.h declares it (a list of the caller's own)"""
    return list(_declared(name))


BF16, F32, FP8, F16 = fa.FA_DTYPE_BF16, fa.FA_DTYPE_F32, fa.FA_DTYPE_FP8_E4M3, fa.FA_DTYPE_F16
FA_ERR = {name: int(code) for name, code in re.findall(r"\bFA_ERR_(\w+)\s*=\s*(-\d+)", _header())}
NULL_POINTER, MISALIGNED, BAD_SHAPE, BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_STRIDE = (FA_ERR[n] for n in (
    "NULL_POINTER", "MISALIGNED", "BAD_SHAPE", "UNSUPPORTED_DHEAD", "UNSUPPORTED_DTYPE", "BAD_SCALE", "BAD_STRIDE"))
CAP = fa.FA_DECODE_MAX_SPLITS
TILE = 128

# short key of the tests -> the header's names for it.  `Sq` is the row count of whichever call (uniform, ragged, append); `T` says
# totalQ alone.  A call that is given two keys for one parameter, or none, is refused (c_call)
KEYS = {
    "Q": ("Q",), "K": ("K", "Kpool"), "V": ("V", "Vpool"), "O": ("O",), "LSE": ("LSE",), "Kn": ("Knew",), "Vn": ("Vnew",),
    "cu": ("cuSeqlensQ",), "lens": ("kvLens",), "table": ("blockTable",), "kd": ("kDescale",), "vd": ("vDescale",), "sinks": ("sinks",),
    "ws": ("workspace",), "B": ("batchSize",), "H": ("numHeads",), "Hkv": ("numHeadsKV",), "Sq": ("seqLenQ", "totalQ", "seqLenNew"),
    "T": ("totalQ",), "Sk": ("seqLenK",), "P": ("numPages",), "page": ("pageSize",), "maxp": ("maxPagesPerSeq",), "ts": ("tableStride",),
    "d": ("dHead",), "scale": ("scale",), "causal": ("is_causal",), "dtype": ("dtype",), "kv": ("kv_dtype",), "o": ("o_dtype",),
    "ns": ("numSplits",), "W": ("windowSize",), "sQ": ("sQ",), "sK": ("sK",), "sV": ("sV",), "sO": ("sO",), "sKn": ("sKnew",),
    "sVn": ("sVnew",), "stream": ("stream",), "plan": ("plan",),
    # flash_attention_rope_append*
    "Qo": ("Qout",), "cs": ("cosSin",), "rot": ("rotDim",), "maxpos": ("maxPos",), "il": ("interleaved",), "sQo": ("sQout",),
    # flash_attention_tree*
    "tree": ("treeMask",),
}
STRIDES = ("sQ", "sK", "sV", "sO", "sKnew", "sVnew", "sQout")


def c_call(symbol, values):
    """`symbol` of the library on the arguments `values` names: every parameter the header declares is looked up under its short key
    (KEYS).  `strides` = the symbol's fa_strides* parameters together, in declared order.  A declared parameter without a value is
    an error, never a default: a parameter added to the header breaks the callers loudly.  Keys the symbol does not declare are
    ignored, so that one dict serves an entry point and its siblings (contiguous / paged, with and without windowSize or sinks)"""
    values = dict(values)
    together = values.pop("strides", None)
    unknown = set(values) - set(KEYS)
    assert not unknown, (symbol, sorted(unknown))
    params = _declared(symbol)
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


def aligned_host_pointer():
    """(buffer, a 16-byte aligned address inside it): keep the buffer alive as long as the address is used"""
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def host_call(symbol, ok, host=None):
    """-> (call, p): call(**overrides) is `symbol` on the aligned host pointer p -- every tensor, cuSeqlensQ, the block table and the
    cos / sin table at p; no LSE, lengths, descales, workspace, stream or strides (as many NULLs as the symbol declares fa_strides*)
    -- and the ints of `ok`, each overridden by name.  `symbol=` in the overrides calls a sibling on the same arguments.  Calls that
    share memory pass one `host` = aligned_host_pointer()"""
    buf, p = host or aligned_host_pointer()
    base = dict(dict(Q=p, K=p, V=p, O=p, Kn=p, Vn=p, Qo=p, cs=p, cu=p, table=p, LSE=None, lens=None, kd=None, vd=None, ws=None, stream=None),
                **ok)

    def call(symbol=symbol, _keep=buf, **overrides):
        no_strides = [None] * sum(n in STRIDES for n in _declared(symbol))
        return c_call(symbol, dict(base, strides=no_strides) | overrides)

    return call, p


def host_calls(*symbols_and_oks):
    """(symbol, ok), ... -> (a host_call of each, ..., p), all on one aligned host pointer p"""
    host = aligned_host_pointer()
    return (*(host_call(symbol, ok, host)[0] for symbol, ok in symbols_and_oks), host[1])


def plan_call(symbol, B, H, Hkv, Sq, Sk, d, o=F32, ns=0, W=None, null_plan=False):
    """-> (return code, the fa_decode_plan as a dict) of a plan function; W for the _window ones; null_plan passes plan = NULL"""
    p = fa.FaDecodePlan()
    values = dict(B=B, H=H, Hkv=Hkv, Sq=Sq, Sk=Sk, d=d, o=o, ns=ns, plan=None if null_plan else ctypes.byref(p))
    rc = c_call(symbol, values if W is None else dict(values, W=W))
    return rc, {k: getattr(p, k) for k, _ in fa.FaDecodePlan._fields_}


def tiles(n):
    return -(-n // TILE)


class MetaTensor:
    """a tensor's metadata with is_cuda = True: the binding's checks run, nothing is launched"""
    is_cuda = True

    def __init__(self, t, device="cuda:0"):
        self.shape, self.dtype, self.dim, self.stride, self.device = t.shape, t.dtype, t.dim, t.stride, device
        self.is_contiguous = t.is_contiguous
        self.unsqueeze = lambda n: MetaTensor(t.unsqueeze(n), device)
        self.transpose = lambda a, b: MetaTensor(t.transpose(a, b), device)
