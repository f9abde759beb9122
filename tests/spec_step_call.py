"""What the tests of flash_attention_rope_append_pos* and flash_attention_kv_accept* share besides the reference
(tests/spec_step_check.py; no tests in here): the calls BY NAME of tests/abi_decl.py (c_call), with the short keys of the four new
parameters, and device-tensor launchers in the manner of tests/rope_call.py.

* `rope_pos(...)`: rope_call.launch with `pos` (int32 device tensor [B, Sq]) -- the _pos entry point of the form.
* `accept(...)`: flash_attention_kv_accept* on device caches (integer dtypes as everywhere: int16 bf16 patterns, uint8 e4m3fn bytes).
"""
import ctypes

import torch

import abi_decl
from abi_decl import BF16, FP8, c_call, fa
from rope_call import _geometry, _ptr, strides3

# the short keys of the parameters the four entry points add (abi_decl.c_call refuses a key it does not know)
abi_decl.KEYS.update(pos=("posOffsets",), idx=("acceptIdx",), nacc=("acceptLens",), draft=("seqLenDraft",))

ROPE_POS = {False: "flash_attention_rope_append_pos", True: "flash_attention_rope_append_paged_pos"}
ROPE_TWIN = {False: "flash_attention_rope_append", True: "flash_attention_rope_append_paged"}
ACCEPT = {False: "flash_attention_kv_accept", True: "flash_attention_kv_accept_paged"}
APPEND = {False: "flash_attention_kv_append", True: "flash_attention_kv_append_paged"}


def _stream(stream):
    return ctypes.c_void_p((torch.cuda.current_stream() if stream is None else stream).cuda_stream)


def rope_pos(Q, Kn, Vn, Qo, K, V, cs, pos, lens=None, il=False, kd=None, vd=None, block_table=None, stream=None, check=True):
    """flash_attention_rope_append_pos / _paged_pos on device tensors; pos = None: the twin without offsets"""
    assert K.dtype in (torch.int16, torch.uint8) and V.dtype == K.dtype and cs.dtype == torch.float32 and cs.is_contiguous()
    assert pos is None or (pos.dtype == torch.int32 and pos.is_contiguous() and tuple(pos.shape) == (Q.shape[0], Q.shape[2]))
    keep = [strides3(Q), strides3(Kn), strides3(Vn), strides3(Qo), strides3(K), strides3(V)]
    values = dict(Q=Q.data_ptr(), Kn=Kn.data_ptr(), Vn=Vn.data_ptr(), Qo=Qo.data_ptr(), K=K.data_ptr(), V=V.data_ptr(), cs=cs.data_ptr(),
                  lens=_ptr(lens), kd=_ptr(kd), vd=_ptr(vd), B=Q.shape[0], H=Q.shape[1], Hkv=Kn.shape[1], Sq=Q.shape[2], d=Q.shape[-1],
                  rot=cs.shape[1], maxpos=cs.shape[0], il=int(il), dtype=BF16, kv=FP8 if K.dtype == torch.uint8 else BF16,
                  strides=[ctypes.byref(s) for s in keep], stream=_stream(stream), **_geometry(K, block_table))
    if pos is not None:
        values["pos"] = pos.data_ptr()
    rc = c_call((ROPE_TWIN if pos is None else ROPE_POS)[block_table is not None], values)
    if check:
        assert rc == 0, (rc, fa.error_string(rc))
    return rc


def accept(K, V, idx, nacc, lens=None, block_table=None, stream=None, check=True):
    """flash_attention_kv_accept / _paged on device caches, in place"""
    assert K.dtype in (torch.int16, torch.uint8) and V.dtype == K.dtype
    assert idx.dtype == torch.int32 and idx.is_contiguous() and nacc.dtype == torch.int32 and nacc.is_contiguous()
    keep = [strides3(K), strides3(V)]
    values = dict(K=K.data_ptr(), V=V.data_ptr(), lens=_ptr(lens), idx=idx.data_ptr(), nacc=nacc.data_ptr(), B=idx.shape[0], Hkv=K.shape[1],
                  draft=idx.shape[1], d=K.shape[-1], kv=FP8 if K.dtype == torch.uint8 else BF16, strides=[ctypes.byref(s) for s in keep],
                  stream=_stream(stream), **_geometry(K, block_table))
    rc = c_call(ACCEPT[block_table is not None], values)
    if check:
        assert rc == 0, (rc, fa.error_string(rc))
    return rc
