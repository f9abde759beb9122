"""CPU tests of the grouped-query entry points of the C ABI (flash_attention_gqa, flash_attention_backward_gqa): the symbols exist
with the declared signatures, an invalid K/V head count is rejected before anything is launched (fake aligned host pointers: no GPU
is touched), every other bad argument gets the code the one-K/V-head-per-query-head entry point gives it, and the Python binding
rejects head counts that do not divide."""
import ctypes

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import BAD_SHAPE, BF16, F16, F32, FP8, aligned_host_pointer, declared_parameters  # noqa: E402


def test_gqa_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    assert "flash_attention_gqa" in fa.EXPORTS and "flash_attention_backward_gqa" in fa.EXPORTS
    assert L.flash_attention_gqa is not None and L.flash_attention_backward_gqa is not None
    # each is its one-K/V-head-per-query-head twin with numHeadsKV after numHeads, and nothing else changed
    fwd, ex = declared_parameters("flash_attention_gqa"), declared_parameters("flash_attention_ex")
    assert fwd == ex[:ex.index("numHeads") + 1] + ["numHeadsKV"] + ex[ex.index("numHeads") + 1:]
    bwd, mha = declared_parameters("flash_attention_backward_gqa"), declared_parameters("flash_attention_backward")
    assert bwd == mha[:mha.index("numHeads") + 1] + ["numHeadsKV"] + mha[mha.index("numHeads") + 1:]
    # ... and the binding passes exactly that many arguments, an int where numHeadsKV stands
    for f, twin, params in ((L.flash_attention_gqa, L.flash_attention_ex, fwd), (L.flash_attention_backward_gqa, L.flash_attention_backward, bwd)):
        at = list(f.argtypes)
        k = params.index("numHeadsKV")
        assert len(at) == len(params) and at[k] is ctypes.c_int and at[:k] + at[k + 1:] == list(twin.argtypes)
        assert f.restype is ctypes.c_int


def forward_calls():
    """(gqa, mha): both entry points on the same keyword arguments; mha ignores Hkv"""
    L = fa.lib()
    buf, p = aligned_host_pointer()
    ok = dict(B=1, H=8, Hkv=2, Sq=16, Sk=16, d=64, scale=0.125, causal=False, dtype=BF16, o=F32, flags=0)
    none = [None] * 4

    def gqa(Q=p, K=p, V=p, O=p, LSE=None, strides=none, _keep=buf, **kw):
        a = dict(ok, **kw)
        return L.flash_attention_gqa(Q, K, V, O, LSE, a["B"], a["H"], a["Hkv"], a["Sq"], a["Sk"], a["d"], a["scale"], a["causal"],
                                     a["dtype"], a["o"], *strides, a["flags"], None)

    def mha(Q=p, K=p, V=p, O=p, LSE=None, strides=none, _keep=buf, **kw):
        a = dict(ok, **kw)
        return L.flash_attention_ex(Q, K, V, O, LSE, a["B"], a["H"], a["Sq"], a["Sk"], a["d"], a["scale"], a["causal"],
                                    a["dtype"], a["o"], *strides, a["flags"], None)

    return gqa, mha, p


def backward_calls():
    L = fa.lib()
    buf, p = aligned_host_pointer()
    ok = dict(B=1, H=8, Hkv=2, Sq=16, Sk=16, d=64, scale=0.125, causal=False, dtype=BF16, o=F32, g=F32)
    none = [None] * 8

    def gqa(Q=p, K=p, V=p, O=p, dO=p, LSE=p, dQ=p, dK=p, dV=p, ws=p, strides=none, _keep=buf, **kw):
        a = dict(ok, **kw)
        return L.flash_attention_backward_gqa(Q, K, V, O, dO, LSE, dQ, dK, dV, ws, a["B"], a["H"], a["Hkv"], a["Sq"], a["Sk"], a["d"],
                                              a["scale"], a["causal"], a["dtype"], a["o"], a["g"], *strides, None)

    def mha(Q=p, K=p, V=p, O=p, dO=p, LSE=p, dQ=p, dK=p, dV=p, ws=p, strides=none, _keep=buf, **kw):
        a = dict(ok, **kw)
        return L.flash_attention_backward(Q, K, V, O, dO, LSE, dQ, dK, dV, ws, a["B"], a["H"], a["Sq"], a["Sk"], a["d"],
                                          a["scale"], a["causal"], a["dtype"], a["o"], a["g"], *strides, None)

    return gqa, mha, p


# numHeadsKV: zero, negative, not a divisor of numHeads (larger than it included)
BAD_HEAD_COUNTS = [(8, 0), (8, -1), (8, -8), (8, 3), (8, 5), (8, 16), (6, 4), (1, 2)]


@pytest.mark.parametrize("H,Hkv", BAD_HEAD_COUNTS)
def test_forward_rejects_an_invalid_kv_head_count_before_any_launch(H, Hkv):
    gqa, _, _ = forward_calls()
    # (the pointers are host memory and there may be no device: anything but a validation code would mean a launch was tried)
    assert gqa(H=H, Hkv=Hkv) == BAD_SHAPE
    assert gqa(H=H, Hkv=Hkv, dtype=F32, d=256) == BAD_SHAPE and gqa(H=H, Hkv=Hkv, dtype=FP8, d=128, o=BF16) == BAD_SHAPE
    assert gqa(H=H, Hkv=Hkv, causal=True, Sq=4096, Sk=4096, d=128) == BAD_SHAPE


@pytest.mark.parametrize("H,Hkv", BAD_HEAD_COUNTS)
def test_backward_rejects_an_invalid_kv_head_count_before_any_launch(H, Hkv):
    gqa, _, _ = backward_calls()
    assert gqa(H=H, Hkv=Hkv) == BAD_SHAPE
    assert gqa(H=H, Hkv=Hkv, causal=True, Sq=4096, Sk=4096, d=128, o=BF16, g=BF16) == BAD_SHAPE


def test_forward_error_codes_match_the_mha_entry_point():
    gqa, mha, p = forward_calls()
    bad = fa.FaStrides(64, 16, 8)            # strideS < d
    mis = fa.FaStrides(1024, 66, 66)         # 132-byte bf16 rows, 264-byte fp32 rows: not multiples of 16 bytes
    cases = [dict(Q=None), dict(K=None), dict(V=None), dict(O=None),                                         # -1
             dict(Q=p + 8), dict(K=p + 4), dict(V=p + 2), dict(O=p + 8), dict(LSE=p + 4),                    # -2
             dict(B=0), dict(B=-1), dict(H=0, Hkv=0), dict(Sq=0), dict(Sk=0), dict(d=0), dict(Sq=(1 << 24) + 1),
             dict(Sk=(1 << 24) + 1), dict(Sk=1 << 23, d=128),                                                # -3
             dict(d=512), dict(d=12), dict(dtype=FP8, d=144), dict(dtype=FP8, d=24), dict(dtype=F32, d=3),   # -4
             dict(dtype=9), dict(dtype=F16), dict(o=FP8), dict(o=7),                                         # -5
             dict(scale=float("nan")), dict(scale=float("inf")), dict(dtype=FP8, d=64, scale=-1.0),          # -6
             dict(flags=4), dict(flags=3), dict(flags=1, d=96), dict(flags=1, dtype=F32), dict(flags=2, dtype=F32),
             dict(flags=1, scale=-0.5)]                                                                      # -8
    for i in range(4):
        for s in (bad, mis):
            st = [None] * 4
            st[i] = ctypes.byref(s)
            cases.append(dict(strides=st))                                                                   # -7
    seen = set()
    for kw in cases:
        want = mha(**kw)
        assert want < 0, kw                                       # each IS a bad argument
        assert gqa(**kw) == want, kw                              # grouped (H 8, Hkv 2) ...
        assert gqa(**dict(dict(Hkv=kw.get("H", 8)), **kw)) == want, kw   # ... and with numHeadsKV = numHeads
        seen.add(want)
    assert seen == {-1, -2, -3, -4, -5, -6, -7, -8}


def test_backward_error_codes_match_the_mha_entry_point():
    gqa, mha, p = backward_calls()
    bad = fa.FaStrides(64, 16, 8)
    mis = fa.FaStrides(1024, 66, 66)
    cases = [{name: None} for name in ("Q", "K", "V", "O", "dO", "LSE", "dQ", "dK", "dV", "ws")]
    cases += [{name: p + 8} for name in ("Q", "K", "V", "O", "dO", "LSE", "dQ", "dK", "dV", "ws")]
    cases += [dict(B=0), dict(B=-1), dict(H=0, Hkv=0), dict(Sq=0), dict(Sk=0), dict(d=0), dict(Sq=(1 << 24) + 1), dict(Sk=1 << 24),
              dict(Sk=1 << 23, d=128),
              dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=0.0), dict(scale=-0.1),
              dict(dtype=F32), dict(dtype=FP8), dict(dtype=F16), dict(dtype=9), dict(o=F16), dict(o=FP8), dict(g=F16), dict(g=FP8)]
    cases += [dict(d=d) for d in (16, 32, 80, 96, 120, 136, 256)]
    for i in range(8):
        for s in (bad, mis):
            st = [None] * 8
            st[i] = ctypes.byref(s)
            cases.append(dict(strides=st))
    seen = set()
    for kw in cases:
        want = mha(**kw)
        assert want < 0, kw
        assert gqa(**kw) == want, kw
        assert gqa(**dict(dict(Hkv=kw.get("H", 8)), **kw)) == want, kw
        seen.add(want)
    assert seen == {-1, -2, -3, -4, -5, -6, -7}


def test_plans_describe_a_grouped_call_by_its_query_heads():
    """the work units are (query head, query block): the plan of a grouped-query call is the plan of its query heads"""
    e, m = fa.plan_ex(8, 16, 4096, 4096, 128, True, BF16, F32, 0)
    assert m["grid"] == 256 and e["q_blocks"] + m["q_blocks"] == 16 and e["unit_lists"] == 1
    assert fa.plan(2, 8, 512, 256, False, BF16, F32)["kernel_id"] == 0


def test_workspace_depends_on_the_query_heads_only():
    up = lambda n: (n + 255) // 256 * 256
    assert fa.backward_workspace_size(2, 8, 300, 128) == up(4 * 2 * 8 * 300) + up(4 * 2 * 8 * 300 * 128)


def test_binding_rejects_head_counts_that_do_not_divide():
    torch = pytest.importorskip("torch")
    q = torch.zeros(2, 8, 16, 64, dtype=torch.bfloat16)
    lse = torch.zeros(2, 8, 16)

    class T:
        """the shape check comes after the device check: a stand-in that claims to be a device tensor gets that far, no further"""
        is_cuda = True

        def __init__(self, t):
            self.shape, self.dtype, self.dim = t.shape, t.dtype, t.dim

    for shape in ((2, 3, 16, 64), (2, 16, 16, 64), (2, 0, 16, 64), (1, 2, 16, 64), (2, 2, 16, 128)):
        k = T(torch.zeros(shape, dtype=torch.bfloat16))
        with pytest.raises(ValueError, match="Hkv dividing H"):
            fa.flash_attention(T(q), k, k)
        with pytest.raises(ValueError, match="Hkv dividing H"):
            fa.flash_attention_backward(T(q), k, k, T(q.float()), T(q.float()), T(lse))
    # a grouped shape passes the shape check and, on host tensors, stops at the device check: no CPU fallback
    k = torch.zeros(2, 2, 16, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention(q, k, k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_backward(q, k, k, q.float(), q.float(), lse)
