"""CPU tests of the backward pass's C ABI: the symbols exist, the workspace size follows its formula, and every invalid argument
is rejected with the forward's error codes before anything is launched (fake aligned pointers: no GPU is touched)."""
import ctypes

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import BF16, F16, F32, FP8  # noqa: E402


def test_backward_symbols_are_exported():
    L = fa.lib()
    assert "flash_attention_backward" in fa.EXPORTS and "flash_attention_backward_workspace_size" in fa.EXPORTS
    assert L.flash_attention_backward is not None and L.flash_attention_backward_workspace_size is not None


@pytest.mark.parametrize("B,H,Sq,d", [(1, 1, 1, 64), (2, 3, 77, 128), (8, 16, 4096, 128), (1, 2, 1000, 64)])
def test_workspace_size_formula(B, H, Sq, d):
    up = lambda n: (n + 255) // 256 * 256
    assert fa.backward_workspace_size(B, H, Sq, d) == up(4 * B * H * Sq) + up(4 * B * H * Sq * d)
    assert fa.backward_workspace_size(B, H, Sq, d) % 256 == 0


def test_workspace_size_of_invalid_shapes_is_zero():
    assert fa.backward_workspace_size(0, 1, 16, 64) == 0 and fa.backward_workspace_size(1, 1, -1, 64) == 0


def test_backward_validation_happens_before_any_launch():
    L = fa.lib()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(B=1, H=1, Sq=16, Sk=16, d=64, scale=0.125, causal=False, dtype=BF16, o=F32, g=F32)
    none = [None] * 8

    def call(Q=p, K=p, V=p, O=p, dO=p, LSE=p, dQ=p, dK=p, dV=p, ws=p, strides=none, **kw):
        a = dict(ok, **kw)
        return L.flash_attention_backward(Q, K, V, O, dO, LSE, dQ, dK, dV, ws, a["B"], a["H"], a["Sq"], a["Sk"], a["d"], a["scale"],
                                          a["causal"], a["dtype"], a["o"], a["g"], *strides, None)

    for name in ("Q", "K", "V", "O", "dO", "LSE", "dQ", "dK", "dV", "ws"):
        assert call(**{name: None}) == -1, name                               # FA_ERR_NULL_POINTER
        assert call(**{name: p + 8}) == -2, name                              # FA_ERR_MISALIGNED
    assert call(Sq=0) == -3 and call(Sk=0) == -3 and call(B=-1) == -3 and call(H=0) == -3 and call(Sq=(1 << 24) + 1) == -3
    assert call(d=0) == -3                                                    # FA_ERR_BAD_SHAPE
    assert call(scale=float("nan")) == -6 and call(scale=float("inf")) == -6 and call(scale=0.0) == -6 and call(scale=-0.1) == -6
    assert call(dtype=F32) == -5 and call(dtype=FP8) == -5 and call(dtype=F16) == -5 and call(dtype=9) == -5
    assert call(o=F16) == -5 and call(o=FP8) == -5 and call(g=F16) == -5 and call(g=FP8) == -5
    for d in (16, 32, 80, 96, 120, 136, 256):
        assert call(d=d) == -4, d                                             # FA_ERR_UNSUPPORTED_DHEAD
    bad = fa.FaStrides(64, 16, 8)                                             # strideS < d
    for i in range(8):
        st = [None] * 8
        st[i] = ctypes.byref(bad)
        assert call(strides=st) == -7, i                                      # FA_ERR_BAD_STRIDE, whichever tensor
    mis = fa.FaStrides(1024, 68, 68)                                          # 136-byte bf16 rows: not a multiple of 16 bytes
    assert call(strides=[ctypes.byref(mis)] + [None] * 7) == -7
    # the forward's per-head extent limit on K / V (32-bit buffer offsets on the MFMA paths)
    assert call(Sk=(1 << 24)) == -3 and call(Sk=1 << 23, d=128) == -3
    assert "unknown flash_attention error" not in fa.error_string(-7)


def test_backward_binding_has_no_cpu_fallback():
    torch = pytest.importorskip("torch")
    x = torch.zeros(1, 1, 16, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_backward(x, x, x, x.float(), x.float(), torch.zeros(1, 1, 16))
