"""What the tests of flash_attention_rope_append* share besides the reference (tests/rope_check.py; no tests in here): device-tensor
launchers over the calls BY NAME of tests/abi_decl.py (c_call; the host-pointer calls of the ladders are abi_decl.host_calls).

* `launch(...)`: a call on device tensors -- the form (contiguous / paged, uniform / ragged) from which arguments are given, the
  strides from the tensors, the cache type from the caches' integer dtype (int16: bf16 patterns, uint8: e4m3fn bytes).
* `twin(...)`: flash_attention_kv_append* of the same form on the same live device tensors.  (memory_contract.append_call is not this:
  it describes a call on CPU data for the placement harness, which allocates, guards and compares; this one launches.)
"""
import ctypes

import torch

from abi_decl import BF16, FP8, c_call, fa

ROPE = {(False, False): "flash_attention_rope_append", (True, False): "flash_attention_rope_append_paged",
        (False, True): "flash_attention_rope_append_varlen", (True, True): "flash_attention_rope_append_paged_varlen"}
TWIN = {k: v.replace("rope_append", "kv_append") for k, v in ROPE.items()}


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
    rc = c_call(TWIN[block_table is not None, ragged], values)
    assert rc == 0, (rc, fa.error_string(rc))
