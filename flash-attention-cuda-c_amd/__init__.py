"""Host-side binding of the MI355X FlashAttention forward path.

The product is ``libflash_attention.so`` (hand-written HIP for gfx950 behind the C ABI declared in
``include/flash_attention.h``).  This module is the thin Python mirror of the reference's two
entry points for that path:

* ``flash_attention(Q, K, V, O, ...)`` -- the launch signature of
  ``twoLoaderMhaFlashAttentionKernel`` (reference ``kernels/FlashAttention.cuh:59-63``; launched at
  ``tests/main.cu:60-61``): dense ``[B, H, S, d]`` device tensors, ``scale``, ``is_causal``.
* ``flash_attention_backward(Q, K, V, O, dO, lse)`` -- dQ, dK, dV of that forward (bf16 inputs, d = 64 / 128), and
  ``attention(Q, K, V)``, the forward as a differentiable ``torch.autograd.Function``.
  All three accept grouped-query attention: K, V ``[B, Hkv, Sk, d]`` with Hkv dividing H; query head h attends K/V head
  ``h // (H // Hkv)`` (``repeat_interleave(H // Hkv, dim=1)`` without the copy), and dK, dV come back shaped like K, V.
* ``flash_attention_decode(Q, K, V, kv_lens)`` -- split-KV decode: 1 .. 16 new query rows per sequence against a long bf16 K/V
  cache, per-sequence lengths in a device tensor, bottom-right-aligned causal mask (``decode_plan``, ``decode_workspace_size``).
* ``flash_attention_decode_paged(Q, K_pool, V_pool, block_table, kv_lens)`` -- the same against paged caches: pools of fixed-size
  pages ``[P, Hkv, page, d]`` and an int32 block table ``[B, max_pages]``, read on the device.  Both also take fp8
  (``torch.float8_e4m3fn``) K/V caches under a bf16 Q, with per-K/V-head ``k_descale`` / ``v_descale``: half the bytes per token.
  Both take ``window=W``: a sliding window, every row sees at most the last W keys up to its own position.
* ``flash_attention_extend(Q, K, V, kv_lens)`` / ``flash_attention_extend_paged(Q, K_pool, V_pool, block_table, kv_lens)`` --
  chunked prefill against the same caches, all four forms: any number of new rows up to the capacity, decode's mask and
  arithmetic (``extend_plan``); ``flash_attention_extend_window`` / ``flash_attention_extend_paged_window`` add ``window=W``.
* ``flash_attention_extend_varlen(Q, K, V, cu_seqlens_q, kv_lens)`` / ``flash_attention_extend_paged_varlen(Q, K_pool, V_pool,
  block_table, cu_seqlens_q, kv_lens)`` -- RAGGED chunked prefill: every sequence its own number of new rows (decode rows, chunks,
  idle slots in one call), Q and O packed by token ``[T, H, d]``, the offsets read on the device (``extend_varlen_plan``);
  ``flash_attention_extend_varlen_window`` / ``flash_attention_extend_paged_varlen_window`` add ``window=W``; and
  ``kv_cache_append_varlen`` / ``kv_cache_append_paged_varlen``, the append of such a batch's new rows.
* ``kv_cache_append(K_new, V_new, K_cache, V_cache, kv_lens)`` / ``kv_cache_append_paged(..., block_table, kv_lens)`` -- the write
  side of those caches: the last Sq rows of every sequence, bf16, copied into a bf16 cache or quantised (divide by the per-head
  descale, saturate, round to nearest even) into an fp8 one, in place, positions and pages found on the device.
* ``rope_cache_append(Q, K_new, V_new, K_cache, V_cache, cos_sin, kv_lens)`` and its ``_paged`` / ``_varlen`` / ``_paged_varlen``
  forms -- the append with the rotary embedding fused in: K rotated at its cache positions into the cache, V appended, the step's Q
  rotated at the same positions, one launch (``rope_table`` makes the cos / sin table).
* ``flash_attention_tree(Q, K, V, tree_mask, kv_lens)`` / ``flash_attention_tree_paged(Q, K_pool, V_pool, block_table, tree_mask,
  kv_lens)`` -- tree-masked verification of a speculative draft: up to 64 draft nodes per sequence, already appended, each row seeing
  the cached prefix and the nodes its 64-bit mask word names (``tree_mask_from_parents``, ``tree_depths``, ``tree_plan``).
* ``flash_attention_cascade_decode(Q, K_shared, V_shared, K, V, shared_len, kv_lens)`` / ``flash_attention_cascade_decode_paged(Q,
  K_pool, V_pool, shared_table, block_table, shared_len, kv_lens)`` -- shared-prefix (cascade) decode: one prefix every sequence of the
  batch sees in full, read once per row block of the whole batch, then each sequence's own suffix (``cascade_plan``).
* ``multi_head_attention(Q, K, V, num_heads)`` -- the reference's Python oracle API
  (``check.py:4-25``): ``(B, S, d_model)`` tensors; the ``(B,S,H,d_k) -> (B,H,S,d_k)`` transposes of
  ``check.py:14-16,24`` are done by strides inside the kernel, not by copies.

PyTorch is used only for device memory and streams.  There is NO fallback: if the shared library
is missing or the tensors are not on a GPU the call raises.  (The directory name contains '-', so
the package is loaded through ``__graft_entry__.load_package()`` under the module name
``flash_attention_cuda_c_amd``.)
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FA_LIB_PATH: another build of the SAME library (the host-sanitizer build of `make asan`); there is still no other implementation
LIB_PATH = os.environ.get("FA_LIB_PATH") or os.path.join(_HERE, "libflash_attention.so")

FA_DTYPE_F32, FA_DTYPE_BF16, FA_DTYPE_FP8_E4M3, FA_DTYPE_F16 = 0, 1, 2, 3
FA_FLAG_F16_WEIGHTS = 1     # flash_attention_ex: softmax weights rounded to fp16 on every row (bf16 inputs, d = 64 / 128)
FA_FLAG_BF16_WEIGHTS = 2    # ... to bf16 on every row; flags = 0: fp16 on the rows that see fewer than FA_EARLY_KEYS keys, bf16 elsewhere
FA_EARLY_KEYS = 1024
FA_DECODE_MAX_Q = 16        # flash_attention_decode: most new query rows per sequence
FA_DECODE_MAX_SPLITS = 64   # ... and the cap of num_splits
FA_DECODE_MAX_WORKGROUPS = 1 << 24   # the K/V-cache calls: plan grid, and rows of O under num_splits > 1, stay below it (FA_ERR_BAD_SHAPE)
FA_VARLEN_MAX_BATCH = 1024  # flash_attention_extend_varlen, kv_cache_append_varlen: most sequences per call
FA_TREE_MAX_Q = 64          # flash_attention_tree: most draft nodes per sequence (one uint64 mask word per node)

# every symbol include/flash_attention.h declares
EXPORTS = ("flash_attention", "flash_attention_strided", "flash_attention_lse", "flash_attention_cross", "flash_attention_ex", "flash_attention_weights", "flash_attention_shard_range", "flash_attention_sharded",
           "flash_attention_plan", "flash_attention_plan_ex", "flash_attention_backward", "flash_attention_backward_workspace_size",
           "flash_attention_gqa", "flash_attention_backward_gqa",
           "flash_attention_decode", "flash_attention_decode_plan", "flash_attention_decode_workspace_size",
           "flash_attention_decode_paged", "flash_attention_decode_fp8", "flash_attention_decode_paged_fp8",
           "flash_attention_decode_window", "flash_attention_decode_paged_window", "flash_attention_decode_plan_window",
           "flash_attention_kv_append", "flash_attention_kv_append_paged",
           "flash_attention_extend", "flash_attention_extend_paged", "flash_attention_extend_plan",
           "flash_attention_extend_varlen", "flash_attention_extend_paged_varlen", "flash_attention_extend_varlen_plan",
           "flash_attention_kv_append_varlen", "flash_attention_kv_append_paged_varlen",
           "flash_attention_extend_window", "flash_attention_extend_paged_window", "flash_attention_extend_plan_window",
           "flash_attention_extend_varlen_window", "flash_attention_extend_paged_varlen_window",
           "flash_attention_extend_varlen_plan_window",
           "flash_attention_sink_decode", "flash_attention_sink_decode_paged", "flash_attention_sink_extend",
           "flash_attention_sink_extend_paged", "flash_attention_sink_extend_varlen", "flash_attention_sink_extend_paged_varlen",
           "flash_attention_rope_append", "flash_attention_rope_append_paged", "flash_attention_rope_append_varlen",
           "flash_attention_rope_append_paged_varlen",
           "flash_attention_tree", "flash_attention_tree_paged", "flash_attention_tree_plan",
           "flash_attention_rope_append_pos", "flash_attention_rope_append_paged_pos",
           "flash_attention_kv_accept", "flash_attention_kv_accept_paged",
           "flash_attention_cascade_decode", "flash_attention_cascade_decode_paged", "flash_attention_cascade_plan",
           "flash_attention_mla_decode", "flash_attention_mla_decode_paged", "flash_attention_mla_decode_plan",
           "flash_attention_mla_decode_workspace_size",
           "flash_attention_error_string", "flash_attention_version")

# The C entry point of a K/V-cache call: _SPLIT_SYMBOLS[family, paged, ragged][window > 0][fp8 cache].  Decode has a bf16-only entry
# point and an ``_fp8`` twin; every extend entry point takes both cache types, and so does every ``_window`` one.
_SPLIT_SYMBOLS = {
    ("decode", False, False): (("flash_attention_decode", "flash_attention_decode_fp8"), ("flash_attention_decode_window",) * 2),
    ("decode", True, False): (("flash_attention_decode_paged", "flash_attention_decode_paged_fp8"),
                              ("flash_attention_decode_paged_window",) * 2),
    ("extend", False, False): (("flash_attention_extend",) * 2, ("flash_attention_extend_window",) * 2),
    ("extend", True, False): (("flash_attention_extend_paged",) * 2, ("flash_attention_extend_paged_window",) * 2),
    ("extend", False, True): (("flash_attention_extend_varlen",) * 2, ("flash_attention_extend_varlen_window",) * 2),
    ("extend", True, True): (("flash_attention_extend_paged_varlen",) * 2, ("flash_attention_extend_paged_varlen_window",) * 2),
}
# ... with ``sinks``: _SINK_SYMBOLS[family, paged, ragged], the ``_window`` entry point's signature with ``sinks`` after the descales
_SINK_SYMBOLS = {
    ("decode", False, False): "flash_attention_sink_decode", ("decode", True, False): "flash_attention_sink_decode_paged",
    ("extend", False, False): "flash_attention_sink_extend", ("extend", True, False): "flash_attention_sink_extend_paged",
    ("extend", False, True): "flash_attention_sink_extend_varlen", ("extend", True, True): "flash_attention_sink_extend_paged_varlen",
}
# ... the tree-masked verification calls: _TREE_SYMBOLS[paged], the sinks entry point of decode without is_causal and with ``treeMask``
# after ``sinks``
_TREE_SYMBOLS = {False: "flash_attention_tree", True: "flash_attention_tree_paged"}
# ... _APPEND_SYMBOLS[paged, ragged], and the plan of a family: _PLAN_SYMBOLS[family, ragged][window > 0]
_APPEND_SYMBOLS = {(False, False): "flash_attention_kv_append", (True, False): "flash_attention_kv_append_paged",
                   (False, True): "flash_attention_kv_append_varlen", (True, True): "flash_attention_kv_append_paged_varlen"}
# ... _ROPE_SYMBOLS[paged, ragged]: the append twin with the rotary embedding fused in
_ROPE_SYMBOLS = {(False, False): "flash_attention_rope_append", (True, False): "flash_attention_rope_append_paged",
                 (False, True): "flash_attention_rope_append_varlen", (True, True): "flash_attention_rope_append_paged_varlen"}
# ... the speculative step's write side: _ROPE_POS_SYMBOLS[paged], the uniform rope twin with ``posOffsets`` after ``cosSin``, and
# _ACCEPT_SYMBOLS[paged], the in-cache acceptance of the verified path
_ROPE_POS_SYMBOLS = {False: "flash_attention_rope_append_pos", True: "flash_attention_rope_append_paged_pos"}
_ACCEPT_SYMBOLS = {False: "flash_attention_kv_accept", True: "flash_attention_kv_accept_paged"}
# ... shared-prefix decode: _CASCADE_SYMBOLS[paged], the ``_window`` entry point of decode with the shared cache, sharedLen, the shared
# table and sinks in, two split counts, and no window
_CASCADE_SYMBOLS = {False: "flash_attention_cascade_decode", True: "flash_attention_cascade_decode_paged"}
_PLAN_SYMBOLS = {("decode", False): ("flash_attention_decode_plan", "flash_attention_decode_plan_window"),
                 ("extend", False): ("flash_attention_extend_plan", "flash_attention_extend_plan_window"),
                 ("extend", True): ("flash_attention_extend_varlen_plan", "flash_attention_extend_varlen_plan_window")}


class FaStrides(ctypes.Structure):
    _fields_ = [("strideB", ctypes.c_int64), ("strideH", ctypes.c_int64), ("strideS", ctypes.c_int64)]


class FaLaunchPlan(ctypes.Structure):
    _fields_ = [("q_block_rows", ctypes.c_int), ("kv_block_rows", ctypes.c_int),
                ("threads", ctypes.c_int), ("grid", ctypes.c_int), ("lds_bytes", ctypes.c_int),
                ("kernel_id", ctypes.c_int)]


class FaLaunchPlanEx(ctypes.Structure):
    _fields_ = [("launch", FaLaunchPlan), ("q_blocks", ctypes.c_int), ("first_q_block", ctypes.c_int), ("unit_lists", ctypes.c_int)]


class FaDecodePlan(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("num_splits", "row_blocks", "rows_per_block", "kv_block_rows", "threads", "grid",
                                            "lds_bytes", "combine_grid", "combine_threads")]


class FaCascadePlan(ctypes.Structure):
    _fields_ = [("shared", FaDecodePlan), ("unique", FaDecodePlan), ("num_splits", ctypes.c_int)]


class FlashAttentionError(RuntimeError):
    def __init__(self, code: int, text: str):
        super().__init__(f"flash_attention failed with code {code}: {text}")
        self.code = code


_lib = None


def lib() -> ctypes.CDLL:
    """Load libflash_attention.so (in-tree build).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} not built: run `make` (or __graft_entry__.build()); there is no fallback path")
        L = ctypes.CDLL(LIB_PATH)
        vp, i, f, b = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_bool
        L.flash_attention.argtypes = [vp, vp, vp, vp, i, i, i, i, f, b, i, i, vp]
        L.flash_attention.restype = i
        sp = ctypes.POINTER(FaStrides)
        L.flash_attention_strided.argtypes = [vp, vp, vp, vp, i, i, i, i, f, b, i, i, sp, sp, sp, sp, vp]
        L.flash_attention_strided.restype = i
        L.flash_attention_lse.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, f, b, i, i, vp]
        L.flash_attention_lse.restype = i
        L.flash_attention_cross.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, f, b, i, i, sp, sp, sp, sp, vp]
        L.flash_attention_cross.restype = i
        L.flash_attention_ex.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, f, b, i, i, sp, sp, sp, sp, ctypes.c_uint, vp]
        L.flash_attention_ex.restype = i
        L.flash_attention_gqa.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, f, b, i, i, sp, sp, sp, sp, ctypes.c_uint, vp]
        L.flash_attention_gqa.restype = i
        L.flash_attention_weights.argtypes = [vp, vp, vp, vp, i, i, i, i, i, f, b, i, sp, sp, vp]
        L.flash_attention_weights.restype = i
        ip, pp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)
        L.flash_attention_shard_range.argtypes = [i, i, i, ip, ip]
        L.flash_attention_shard_range.restype = i
        L.flash_attention_sharded.argtypes = [i, ip, pp, pp, pp, pp, i, i, i, i, f, b, i, i, pp]
        L.flash_attention_sharded.restype = i
        L.flash_attention_plan.argtypes = [i, i, i, i, b, i, i, ctypes.POINTER(FaLaunchPlan)]
        L.flash_attention_plan.restype = i
        px = ctypes.POINTER(FaLaunchPlanEx)
        L.flash_attention_plan_ex.argtypes = [i, i, i, i, i, b, i, i, ctypes.c_uint, px, px]
        L.flash_attention_plan_ex.restype = i
        L.flash_attention_backward.argtypes = [vp] * 10 + [i, i, i, i, i, f, b, i, i, i] + [sp] * 8 + [vp]
        L.flash_attention_backward.restype = i
        L.flash_attention_backward_gqa.argtypes = [vp] * 10 + [i, i, i, i, i, i, f, b, i, i, i] + [sp] * 8 + [vp]
        L.flash_attention_backward_gqa.restype = i
        L.flash_attention_backward_workspace_size.argtypes = [i, i, i, i]
        L.flash_attention_backward_workspace_size.restype = ctypes.c_size_t
        L.flash_attention_decode_workspace_size.argtypes = [i, i, i, i, i]
        L.flash_attention_decode_workspace_size.restype = ctypes.c_size_t
        # the split-KV and append families, from their parts: the tensors, cuSeqlensQ (ragged) before kvLens, the block table (paged),
        # the descales (every call but the bf16-only decode pair), then the ints with the cache geometry in the middle, kv_dtype next to
        # dtype where there are descales, windowSize after numSplits, the strides and the stream; the sinks entry point of a form is
        # its ``_window`` one with sinks after the descales
        paging = lambda paged: [i, i, i, ctypes.c_int64] if paged else [i]      # numPages, pageSize, maxPagesPerSeq, tableStride / seqLenK
        for (family, paged, ragged), by_window in _SPLIT_SYMBOLS.items():
            for window, by_cache in enumerate(by_window):
                for fp8, name in enumerate(by_cache):
                    both = family == "extend" or bool(window) or bool(fp8)     # the entry point has descales and kv_dtype
                    fns = [(getattr(L, name), 0)] + ([(getattr(L, _SINK_SYMBOLS[family, paged, ragged]), 1)] if window else [])
                    for fn, sink in fns:
                        fn.argtypes = [vp] * 5 + [vp] * ragged + [vp] + [vp] * paged + [vp, vp] * both + [vp] * sink + [vp] + [i] * 4 \
                            + paging(paged) + [i, f, b, i] + [i] * both + [i, i] + [i] * window + [sp] * 4 + [vp]
                        fn.restype = i
        for paged, name in _TREE_SYMBOLS.items():      # sinks and treeMask after the descales; no is_causal; windowSize always
            fn = getattr(L, name)
            fn.argtypes = [vp] * 6 + [vp] * paged + [vp] * 5 + [i] * 4 + paging(paged) + [i, f] + [i] * 5 + [sp] * 4 + [vp]
            fn.restype = i
        L.flash_attention_tree_plan.argtypes = [i] * 9 + [ctypes.POINTER(FaDecodePlan)]
        L.flash_attention_tree_plan.restype = i
        for (paged, ragged), name in _APPEND_SYMBOLS.items():
            fn = getattr(L, name)
            fn.argtypes = [vp] * 4 + [vp] * ragged + [vp] + [vp] * paged + [vp, vp] + [i] * 3 + paging(paged) + [i, i, i] + [sp] * 4 + [vp]
            fn.restype = i
        # the rope twins: Q first, Qout after the new rows, cosSin after the caches; numHeads after batchSize; rotDim, maxPos and
        # interleaved after dHead; sQ first of the strides and sQout after the new rows'
        for (paged, ragged), name in _ROPE_SYMBOLS.items():
            fn = getattr(L, name)
            fn.argtypes = [vp] * 7 + [vp] * ragged + [vp] + [vp] * paged + [vp, vp] + [i] * 4 + paging(paged) + [i] * 6 + [sp] * 6 + [vp]
            fn.restype = i
        for paged, name in _ROPE_POS_SYMBOLS.items():      # posOffsets after cosSin
            fn = getattr(L, name)
            fn.argtypes = [vp] * 8 + [vp] + [vp] * paged + [vp, vp] + [i] * 4 + paging(paged) + [i] * 6 + [sp] * 6 + [vp]
            fn.restype = i
        for paged, name in _ACCEPT_SYMBOLS.items():        # the caches, kvLens, the table (paged), acceptIdx, acceptLens
            fn = getattr(L, name)
            fn.argtypes = [vp] * 3 + [vp] * paged + [vp, vp] + [i] * 3 + paging(paged) + [i, i] + [sp] * 2 + [vp]
            fn.restype = i
        # the cascade pair: Q, the shared K / V and the K / V of the suffixes (paged: the two pools), O, LSE, sharedLen, kvLens, the two
        # tables (paged), the descales, sinks, the workspace; seqLenShared before seqLenK (paged: maxSharedPages before maxPagesPerSeq);
        # two split counts; the shared tensors' strides before K's (paged: the pools' only)
        L.flash_attention_cascade_decode.argtypes = [vp] * 13 + [i] * 7 + [f, b] + [i] * 5 + [sp] * 6 + [vp]
        L.flash_attention_cascade_decode_paged.argtypes = [vp] * 13 + [i] * 8 + [ctypes.c_int64, i, f, b] + [i] * 5 + [sp] * 4 + [vp]
        L.flash_attention_cascade_decode.restype = L.flash_attention_cascade_decode_paged.restype = i
        L.flash_attention_cascade_plan.argtypes = [i] * 10 + [ctypes.POINTER(FaCascadePlan)]
        L.flash_attention_cascade_plan.restype = i
        # the MLA pair: Q, the latent cache (paged: the pool), O, LSE, kvLens, the table (paged), the workspace; no K/V head count;
        # dLatent, dRope where dHead stands; three strides
        for paged in (False, True):
            fn = getattr(L, "flash_attention_mla_decode_paged" if paged else "flash_attention_mla_decode")
            fn.argtypes = [vp] * 5 + [vp] * paged + [vp] + [i] * 3 + paging(paged) + [i, i, f, b, i, i, i] + [sp] * 3 + [vp]
            fn.restype = i
        L.flash_attention_mla_decode_plan.argtypes = [i] * 8 + [ctypes.POINTER(FaDecodePlan)]
        L.flash_attention_mla_decode_plan.restype = i
        L.flash_attention_mla_decode_workspace_size.argtypes = [i, i, i, i, i]
        L.flash_attention_mla_decode_workspace_size.restype = ctypes.c_size_t
        for by_window in _PLAN_SYMBOLS.values():
            for window, name in enumerate(by_window):
                fn = getattr(L, name)
                fn.argtypes = [i] * 8 + [i] * window + [ctypes.POINTER(FaDecodePlan)]
                fn.restype = i
        L.flash_attention_error_string.argtypes = [i]
        L.flash_attention_error_string.restype = ctypes.c_char_p
        L.flash_attention_version.argtypes = []
        L.flash_attention_version.restype = ctypes.c_char_p
        _lib = L
    return _lib


def version() -> str:
    return lib().flash_attention_version().decode()


def error_string(code: int) -> str:
    return lib().flash_attention_error_string(int(code)).decode()


def _check(code: int):
    if code != 0:
        raise FlashAttentionError(code, error_string(code))


def _dtype_code(t):
    import torch
    table = {torch.float32: FA_DTYPE_F32, torch.bfloat16: FA_DTYPE_BF16, torch.float16: FA_DTYPE_F16}
    if hasattr(torch, "float8_e4m3fn"):
        table[torch.float8_e4m3fn] = FA_DTYPE_FP8_E4M3
    if t not in table:
        raise TypeError(f"unsupported dtype {t}")
    return table[t]


def _default_out_dtype(in_dtype):
    """fp32 in -> fp32 out (the reference's float* O); fp8 in -> bf16 out; otherwise the input type."""
    import torch
    if in_dtype == torch.float32:
        return torch.float32
    if in_dtype == getattr(torch, "float8_e4m3fn", None):
        return torch.bfloat16
    return in_dtype


def _stream_ptr(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def plan(batchSize, numHeads, seqLen, dHead, is_causal=False, dtype=FA_DTYPE_BF16, o_dtype=FA_DTYPE_F32):
    """Launch geometry the library will use (counterpart of the reference's helpers.hpp:8-36)."""
    p = FaLaunchPlan()
    _check(lib().flash_attention_plan(batchSize, numHeads, seqLen, dHead, bool(is_causal), dtype, o_dtype,
                                      ctypes.byref(p)))
    return {k: getattr(p, k) for k, _ in FaLaunchPlan._fields_}


def plan_ex(batchSize, numHeads, seqLenQ, seqLenK, dHead, is_causal=False, dtype=FA_DTYPE_BF16, o_dtype=FA_DTYPE_F32, flags=0):
    """The launches a flash_attention_ex() call makes: (early, main) dicts; a launch that does not happen has q_blocks = 0."""
    e, m = FaLaunchPlanEx(), FaLaunchPlanEx()
    _check(lib().flash_attention_plan_ex(batchSize, numHeads, seqLenQ, seqLenK, dHead, bool(is_causal), dtype, o_dtype, flags,
                                         ctypes.byref(e), ctypes.byref(m)))
    conv = lambda x: dict({k: getattr(x.launch, k) for k, _ in FaLaunchPlan._fields_}, q_blocks=x.q_blocks, first_q_block=x.first_q_block, unit_lists=x.unit_lists)
    return conv(e), conv(m)


def flash_attention(Q, K, V, O=None, scale=None, is_causal=False, out_dtype=None, stream=None, return_lse=False, weights_dtype=None):
    """O = softmax(scale * Q K^T [+ causal mask]) V on [B, H, S, d] device tensors.

    Argument order and meaning follow the reference kernel (Q, K, V, O, batchSize, numHeads,
    seqLen, scale, is_causal -- kernels/FlashAttention.cuh:59-63); batchSize/numHeads/seqLen/dHead
    are read from Q.shape, ``scale`` defaults to 1/sqrt(d) (tests/main.cu:27).  K and V may hold a
    different number of rows than Q (``[B, H, Sk, d]``: the seqLenQ / seqLenK of the reference's first
    API, kernels/FlashAttention.cuh:23); the causal mask stays ``k > q`` on absolute indices.
    Grouped-query attention: K and V may hold fewer heads, ``[B, Hkv, Sk, d]`` with Hkv dividing H; query head h then attends
    K/V head ``h // (H // Hkv)`` (flash_attention_gqa; the result equals the call on ``K.repeat_interleave(H // Hkv, 1)``).
    Asynchronous on ``stream`` (default: torch's current stream).  Returns O, or ``(O, LSE)`` with
    ``return_lse=True`` (LSE: fp32 [B, H, S], natural-log sum of exp(scale * scores) over the visible keys).
    ``weights_dtype`` (bf16 inputs): None = the library default (fp16 softmax weights on the rows that see fewer than
    FA_EARLY_KEYS keys, bf16 weights elsewhere); ``torch.float16`` = FA_FLAG_F16_WEIGHTS (fp16 weights on every row; d = 64
    or 128); ``torch.bfloat16`` = FA_FLAG_BF16_WEIGHTS (bf16 weights on every row: the fastest form; accepted and ignored for
    fp32 / fp8 inputs, which have one form).
    """
    import torch
    if not (Q.is_cuda and K.is_cuda and V.is_cuda):
        raise RuntimeError("flash_attention needs device tensors (no CPU fallback)")
    if Q.dim() != 4 or K.dim() != 4 or K.shape != V.shape or Q.shape[0] != K.shape[0] or Q.shape[3] != K.shape[3] \
            or K.shape[1] < 1 or Q.shape[1] % K.shape[1] != 0:
        raise ValueError("Q must be [B, H, S, d] and K, V [B, Hkv, Sk, d] with Hkv dividing H")
    if not (Q.dtype == K.dtype == V.dtype):
        raise TypeError("Q, K, V must share a dtype")
    B, H, S, d = Q.shape
    Hkv, Sk = K.shape[1:3]
    if scale is None:
        scale = 1.0 / float(d) ** 0.5
    if O is None:
        O = torch.empty((B, H, S, d), dtype=out_dtype or _default_out_dtype(Q.dtype), device=Q.device)
    elif O.shape != Q.shape or not O.is_cuda:
        raise ValueError("O must be a device tensor shaped like Q")
    dense = all(t.is_contiguous() for t in (Q, K, V, O))
    lse = torch.empty((B, H, S), dtype=torch.float32, device=Q.device) if return_lse else None
    common = (float(scale), bool(is_causal), _dtype_code(Q.dtype), _dtype_code(O.dtype))
    ptrs = (Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr())
    flags = 0
    if weights_dtype is not None:
        if weights_dtype == torch.float16:
            flags |= FA_FLAG_F16_WEIGHTS
        elif weights_dtype == torch.bfloat16:
            # bf16 weights are what fp32 / fp8 inputs get anyway (one form each): the request is a no-op there, not an error --
            # the library rejects the FLAG on non-bf16 inputs (FA_ERR_BAD_FLAGS), so it is only set where it selects something
            if Q.dtype == torch.bfloat16:
                flags |= FA_FLAG_BF16_WEIGHTS
        else:
            raise TypeError("weights_dtype must be torch.float16 or torch.bfloat16")
    with torch.cuda.device(Q.device):
        if Hkv != H:
            refs = [ctypes.byref(_strides(t)) for t in (Q, K, V, O)]
            rc = lib().flash_attention_gqa(*ptrs, lse.data_ptr() if lse is not None else None, B, H, Hkv, S, Sk, d, *common, *refs,
                                           flags, _stream_ptr(stream))
        elif flags:
            refs = [ctypes.byref(_strides(t)) for t in (Q, K, V, O)]
            rc = lib().flash_attention_ex(*ptrs, lse.data_ptr() if lse is not None else None, B, H, S, Sk, d, *common, *refs,
                                          flags, _stream_ptr(stream))
        elif dense and Sk == S and lse is not None:
            rc = lib().flash_attention_lse(*ptrs, lse.data_ptr(), B, H, S, d, *common, _stream_ptr(stream))
        elif dense and Sk == S:
            rc = lib().flash_attention(*ptrs, B, H, S, d, *common, _stream_ptr(stream))
        else:
            refs = [ctypes.byref(_strides(t)) for t in (Q, K, V, O)]
            if Sk == S and lse is None:
                rc = lib().flash_attention_strided(*ptrs, B, H, S, d, *common, *refs, _stream_ptr(stream))
            else:
                rc = lib().flash_attention_cross(*ptrs, lse.data_ptr() if lse is not None else None, B, H, S, Sk, d,
                                                 *common, *refs, _stream_ptr(stream))
    _check(rc)
    return (O, lse) if return_lse else O


def shard_range(total_heads, rank, world):
    """[lo, hi) of flattened heads g = b*H + h owned by `rank` of `world` (C ABI twin of shard.shard_heads)."""
    lo, hi = ctypes.c_int(), ctypes.c_int()
    _check(lib().flash_attention_shard_range(total_heads, rank, world, ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def flash_attention_sharded(Qs, Ks, Vs, Os, batchSize, numHeads, scale=None, is_causal=False, streams=None):
    """One host thread, several devices: Qs[r], Ks[r], Vs[r], Os[r] are rank r's dense [hi-lo, S, d] slabs of the
    flattened heads (shard_range), each resident on its own device.  No collective; asynchronous."""
    n = len(Qs)
    S, d = Qs[0].shape[-2:]
    if scale is None:
        scale = 1.0 / float(d) ** 0.5
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    devs = (ctypes.c_int * n)(*[t.device.index for t in Qs])
    st = (ctypes.c_void_p * n)(*[s.cuda_stream if s is not None else None for s in (streams or [None] * n)])
    _check(lib().flash_attention_sharded(n, devs, arr(Qs), arr(Ks), arr(Vs), arr(Os), batchSize, numHeads, S, d, float(scale),
                                         bool(is_causal), _dtype_code(Qs[0].dtype), _dtype_code(Os[0].dtype), st))
    return Os


def attention_weights(Q, K, lse, scale=None, is_causal=False, stream=None):
    """attn[b,h,q,k] = exp(scale * <Q[q], K[k]> - lse[q]) as a dense fp32 [B, H, Sq, Sk] device tensor -- the
    matrix check.py:20,25 returns as ``attn`` -- from the LSE of a ``flash_attention(..., return_lse=True)``
    call.  Inspection path for small sequences (the fused kernel itself never stores it)."""
    import torch
    B, H, S, d = Q.shape
    Sk = K.shape[2]
    if scale is None:
        scale = 1.0 / float(d) ** 0.5
    if Q.stride(3) != 1 or K.stride(3) != 1 or not lse.is_contiguous() or lse.dtype != torch.float32:
        raise ValueError("last dimension must be contiguous; lse must be dense fp32 [B, H, S]")
    P = torch.empty((B, H, S, Sk), dtype=torch.float32, device=Q.device)
    sq, sk = (FaStrides(t.stride(0), t.stride(1), t.stride(2)) for t in (Q, K))
    with torch.cuda.device(Q.device):
        rc = lib().flash_attention_weights(Q.data_ptr(), K.data_ptr(), lse.data_ptr(), P.data_ptr(), B, H, S, Sk, d,
                                           float(scale), bool(is_causal), _dtype_code(Q.dtype), ctypes.byref(sq),
                                           ctypes.byref(sk), _stream_ptr(stream))
    _check(rc)
    return P


def multi_head_attention(Q, K, V, num_heads, is_causal=False, return_attn=False, out_dtype=None):
    """Drop-in for the reference's ``check.py:multi_head_attention(Q, K, V, num_heads)``.

    Q, K, V: (batch, seq_len, d_model) device tensors.  Returns ``(output, attn)`` like check.py:25,
    with output (batch, seq_len, d_model).  The fused kernel never materialises the (B,H,S,S) attention
    matrix, so ``attn`` is None unless ``return_attn=True``, which rebuilds it (fp32) from the kernel's
    log-sum-exp with a second small kernel -- meant for the small shapes check.py's demo prints.
    The head split / merge of check.py:14-16,24 is done with strides: no transpose copies.
    """
    import torch
    if Q.dim() != 3:
        raise ValueError("Q, K, V must be (batch, seq_len, d_model)")
    B, S, dm = Q.shape
    if dm % num_heads != 0:
        raise ValueError("d_model must be divisible by num_heads")
    dk = dm // num_heads                                                 # check.py:11
    out = torch.empty((B, S, dm), device=Q.device, dtype=out_dtype or _default_out_dtype(Q.dtype))
    view = lambda t: t.view(B, S, num_heads, dk).transpose(1, 2)         # check.py:14-16 (views only)
    scale = 1.0 / float(dk) ** 0.5                                       # check.py:19
    if not return_attn:
        flash_attention(view(Q), view(K), view(V), view(out), scale=scale, is_causal=is_causal)
        return out, None
    _, lse = flash_attention(view(Q), view(K), view(V), view(out), scale=scale, is_causal=is_causal, return_lse=True)
    return out, attention_weights(view(Q), view(K), lse, scale=scale, is_causal=is_causal)


def _strides(t):
    if t.stride(3) != 1:
        raise ValueError("last dimension must be contiguous")
    return FaStrides(t.stride(0), t.stride(1), t.stride(2))


def backward_workspace_size(B, H, Sq, d):
    """Bytes of device scratch flash_attention_backward needs."""
    return int(lib().flash_attention_backward_workspace_size(B, H, Sq, d))


def flash_attention_backward(Q, K, V, O, dO, lse, scale=None, is_causal=False, grad_dtype=None, dQ=None, dK=None, dV=None,
                             stream=None):
    """(dQ, dK, dV) of O = softmax(scale * Q K^T [+ causal mask]) V, recomputing the softmax from ``lse`` -- the LSE a
    ``flash_attention(..., return_lse=True)`` call returned with the same Q, K, scale and mask.

    Q, K, V: bf16 [B, H, Sq, d] / [B, Hkv, Sk, d] device tensors, d = 64 or 128, Hkv dividing H (grouped-query attention as in
    ``flash_attention``: dK, dV are shaped like K, V, each the sum over the query heads that share the head); O and dO:
    [B, H, Sq, d] in fp32 or bf16 (one type for both); lse: dense fp32 [B, H, Sq].  Strided views are accepted (last dimension contiguous).  ``grad_dtype`` (fp32 or
    bf16) defaults to the type of O; dQ / dK / dV may be given (shaped like Q / K / V).  The workspace is allocated with torch on
    the tensors' device, on ``stream``, like gradients this call allocates.  Asynchronous on ``stream`` (default: torch's current
    stream); the caller orders its other streams after it, as for any torch kernel.  No CPU fallback."""
    import torch
    if not all(t.is_cuda for t in (Q, K, V, O, dO, lse)):
        raise RuntimeError("flash_attention_backward needs device tensors (no CPU fallback)")
    if Q.dim() != 4 or K.dim() != 4 or K.shape != V.shape or Q.shape[0] != K.shape[0] or Q.shape[3] != K.shape[3] \
            or K.shape[1] < 1 or Q.shape[1] % K.shape[1] != 0 or O.shape != Q.shape or dO.shape != Q.shape:
        raise ValueError("Q, O, dO must be [B, H, Sq, d] and K, V [B, Hkv, Sk, d] with Hkv dividing H")
    if O.dtype != dO.dtype:
        raise TypeError("O and dO must share a dtype")
    B, H, S, d = Q.shape
    Hkv, Sk = K.shape[1:3]
    if lse.shape != (B, H, S) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise ValueError("lse must be dense fp32 [B, H, Sq]")
    if scale is None:
        scale = 1.0 / float(d) ** 0.5
    gd = grad_dtype or O.dtype
    with torch.cuda.device(Q.device):
        s = stream if stream is not None else torch.cuda.current_stream()
        # the workspace (and any gradient allocated here) belongs to the stream the kernels run on: the caching allocator hands a
        # block freed on stream s only to later work on s, which runs after these kernels -- allocated on another stream, the
        # workspace released at return could be reused by that stream while the kernels still read and add into it
        with torch.cuda.stream(s):
            dQ = torch.empty((B, H, S, d), dtype=gd, device=Q.device) if dQ is None else dQ
            dK = torch.empty((B, Hkv, Sk, d), dtype=gd, device=Q.device) if dK is None else dK
            dV = torch.empty((B, Hkv, Sk, d), dtype=gd, device=Q.device) if dV is None else dV
            if dQ.shape != Q.shape or dK.shape != K.shape or dV.shape != K.shape or not (dQ.dtype == dK.dtype == dV.dtype):
                raise ValueError("dQ must be shaped like Q, dK and dV like K, all three of one dtype")
            ws = torch.empty(backward_workspace_size(B, H, S, d), dtype=torch.uint8, device=Q.device)
        st = [_strides(t) for t in (Q, K, V, O, dO, dQ, dK, dV)]
        ptrs = (Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), lse.data_ptr(),
                dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), ws.data_ptr())
        tail = (S, Sk, d, float(scale), bool(is_causal), _dtype_code(Q.dtype), _dtype_code(O.dtype), _dtype_code(dQ.dtype),
                *[ctypes.byref(x) for x in st], _stream_ptr(s))
        if Hkv != H:
            rc = lib().flash_attention_backward_gqa(*ptrs, B, H, Hkv, *tail)
        else:
            rc = lib().flash_attention_backward(*ptrs, B, H, *tail)
    _check(rc)
    return dQ, dK, dV


def _window(window):
    """``window`` of the decode fronts as the C ABI's windowSize: None and 0 = no window"""
    window = 0 if window is None else int(window)
    if window < 0:
        raise ValueError("window must be None, 0 (no window) or a positive number of keys")
    return window


def _split_plan(family, ragged, B, H, Hkv, Sq, Sk, d, o_dtype, num_splits, window):
    """the filled fa_decode_plan of a call, from the family's plan entry point or (a window) its ``_window`` twin"""
    p = FaDecodePlan()
    window = _window(window)
    if family == "tree":      # one plan entry point, the window always among its arguments
        _check(lib().flash_attention_tree_plan(B, H, Hkv, Sq, Sk, d, o_dtype, num_splits, window, ctypes.byref(p)))
        return p
    plain, windowed = _PLAN_SYMBOLS[family, ragged]
    if window:
        _check(getattr(lib(), windowed)(B, H, Hkv, Sq, Sk, d, o_dtype, num_splits, window, ctypes.byref(p)))
    else:
        _check(getattr(lib(), plain)(B, H, Hkv, Sq, Sk, d, o_dtype, num_splits, ctypes.byref(p)))
    return p


def _plan_dict(p):
    return {k: getattr(p, k) for k, _ in FaDecodePlan._fields_}


def decode_plan(B, H, Hkv, Sq, Sk, d, o_dtype=FA_DTYPE_BF16, num_splits=0, window=0):
    """What a flash_attention_decode call launches (fa_decode_plan as a dict); ``num_splits`` 0 = the library's choice.  ``window``
    > 0: the call's sliding window -- the split count then follows from the window's tiles, not the capacity's."""
    return _plan_dict(_split_plan("decode", False, B, H, Hkv, Sq, Sk, d, o_dtype, num_splits, window))


def extend_plan(B, H, Hkv, Sq, Sk, d, o_dtype=FA_DTYPE_BF16, num_splits=0, window=None):
    """What a flash_attention_extend call launches (fa_decode_plan as a dict; ``Sk`` the capacity); ``num_splits`` 0 = the library's
    choice.  ``rows_per_block`` packed rows ``g * Sq + i`` of one K/V head form a row block; ``decode_workspace_size`` serves unchanged.
    ``window`` > 0: the call's sliding window -- the split count then follows from the window's tiles, as in ``decode_plan``."""
    return _plan_dict(_split_plan("extend", False, B, H, Hkv, Sq, Sk, d, o_dtype, num_splits, window))


def extend_varlen_plan(B, H, Hkv, total_q, Sk, d, o_dtype=FA_DTYPE_BF16, num_splits=0, window=None):
    """What a flash_attention_extend_varlen call launches (fa_decode_plan as a dict; ``total_q`` the bound on the packed rows, ``Sk``
    the capacity); ``num_splits`` 0 = the library's choice.  ``row_blocks`` is the host's BOUND on the row blocks of the whole batch,
    ``(G * total_q + B * (rows_per_block - 1)) // rows_per_block``; the workspace is ``decode_workspace_size(1, H, total_q, d, ns)``.
    ``window`` > 0: the call's sliding window (the tiles bound uses ``total_q`` for the row count)."""
    return _plan_dict(_split_plan("extend", True, B, H, Hkv, total_q, Sk, d, o_dtype, num_splits, window))


def tree_plan(B, H, Hkv, Sq, Sk, d, o_dtype=FA_DTYPE_BF16, num_splits=0, window=0):
    """What a flash_attention_tree call launches (fa_decode_plan as a dict): ``decode_plan`` for Sq <= FA_DECODE_MAX_Q draft nodes,
    ``extend_plan`` for 17 .. FA_TREE_MAX_Q, under the same ``window``; ``decode_workspace_size`` serves unchanged."""
    return _plan_dict(_split_plan("tree", False, B, H, Hkv, Sq, Sk, d, o_dtype, num_splits, window))


def decode_workspace_size(B, H, Sq, d, num_splits):
    """Bytes of device scratch flash_attention_decode needs for ``num_splits`` splits as planned (0 for one split)."""
    return int(lib().flash_attention_decode_workspace_size(B, H, Sq, d, num_splits))


def _cu_seqlens(cu_seqlens_q, device_of):
    """the checks of a ragged front's ``cu_seqlens_q``; returns the batch size"""
    import torch
    cu = cu_seqlens_q
    if not getattr(cu, "is_cuda", False) or cu.dtype != torch.int32 or cu.dim() != 1 or cu.shape[0] < 2 or not cu.is_contiguous() \
            or cu.device != device_of.device:
        raise ValueError("cu_seqlens_q must be a dense int32 device tensor [B + 1] on the device of the rows")
    return cu.shape[0] - 1


def _token_view(t, what):
    """a token-packed ``[T, heads, d]`` tensor as the ``[1, heads, T, d]`` view the shared fronts take (no copy)"""
    if t.dim() != 3:
        raise ValueError(f"{what} must be packed by token: [T, heads, d]")
    return t.unsqueeze(0).transpose(1, 2)


def _decode_inputs(name, kv, layout, Q, K, V, k_descale, v_descale, table=None, batch=None):
    """The checks both decode fronts make of Q and the tensors that play K/V (``kv``, ``layout``: their names and shape in the error
    texts; ``table``: the paged front's block table -- pools are not indexed by the batch).  True when the call is the fp8-cache form (bf16 Q,
    e4m3fn K and V); the dtypes and the descales are checked either way."""
    import torch
    if not (Q.is_cuda and K.is_cuda and V.is_cuda and (table is None or table.is_cuda)):
        raise RuntimeError(f"{name} needs device tensors (no CPU fallback)")
    if Q.dim() != 4 or K.dim() != 4 or K.shape != V.shape or (table is None and (Q.shape[0] if batch is None else batch) != K.shape[0]) \
            or Q.shape[3] != K.shape[3] or K.shape[1] < 1 or Q.shape[1] % K.shape[1] != 0:
        raise ValueError(f"Q must be {'[B, H, Sq, d]' if batch is None else '[T, H, d]'} and {kv} {layout} with Hkv dividing H")
    f8 = getattr(torch, "float8_e4m3fn", None)
    fp8 = f8 is not None and Q.dtype == torch.bfloat16 and K.dtype == f8 and V.dtype == f8
    if not fp8 and not (Q.dtype == K.dtype == V.dtype):
        raise TypeError(f"Q, {kv} must share a dtype")
    for what, t in (("k_descale", k_descale), ("v_descale", v_descale)):
        if t is None:
            continue
        if not fp8:
            raise ValueError(f"{what} belongs to an fp8 (float8_e4m3fn) K/V cache under a bf16 Q")
        if getattr(t, "dtype", None) != torch.float32 or not t.is_cuda or t.device != Q.device or tuple(t.shape) != (K.shape[1],) \
                or not t.is_contiguous():
            raise ValueError(f"{what} must be a dense fp32 tensor [Hkv] on the device of Q")
    return fp8


def _table_geometry(block_table, B):
    """(max_pages, table_stride) of a paged front's block table, after its checks"""
    import torch
    t = block_table
    if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != B or t.shape[1] < 1 or t.stride(1) != 1 or (B > 1 and t.stride(0) < t.shape[1]):
        raise ValueError("block_table must be an int32 device tensor [B, max_pages] with a contiguous last dimension")
    return t.shape[1], (t.stride(0) if B > 1 else t.shape[1])


def _cache_geometry(K, block_table, B):
    """(capacity, tables, geometry) of the cache a front got -- ``K`` with its ``block_table`` is a pool, without one the contiguous
    cache: the rows a sequence can hold, the table pointers and the integers the entry point takes for the cache's shape"""
    if block_table is None:
        return K.shape[2], (), (K.shape[2],)
    max_pages, table_stride = _table_geometry(block_table, B)
    return max_pages * K.shape[2], (block_table,), (K.shape[0], K.shape[2], max_pages, table_stride)


def _check_kv_lens(kv_lens, B):
    """the check every cache front makes of its optional ``kv_lens``"""
    import torch
    if kv_lens is not None and (not kv_lens.is_cuda or kv_lens.dtype != torch.int32 or kv_lens.shape != (B,)
                                or not kv_lens.is_contiguous()):
        raise ValueError("kv_lens must be a dense int32 device tensor [B]")


def _split_front(family, Q, K, V, block_table=None, cu_seqlens_q=None, kv_lens=None, scale=None, is_causal=False, out_dtype=None,
                 num_splits=0, return_lse=False, O=None, workspace=None, stream=None, k_descale=None, v_descale=None, window=None,
                 sinks=None, tree_mask=None):
    """Every flash_attention_decode* / flash_attention_extend* front: ``family`` is "decode" or "extend", a ``block_table`` makes the call
    paged (K, V are then the pools) and ``cu_seqlens_q`` ragged (Q -- and O, if given -- are then packed by token: Sq is the bound on
    the packed rows, the batch is cu_seqlens_q's, the LSE is ``[H, T]``, and an O or LSE allocated here is zero-filled).  The checks of the
    tensors, the plan and the workspace for the capacity, then the entry point of _SPLIT_SYMBOLS: the ones that take both cache types
    get the descales and the cache's dtype code, the ``_window`` ones the window.  ``sinks`` (a dense fp32 ``[H]`` tensor on Q's device:
    one attention-sink logit per query head, natural-log units, not scaled; read by the kernel): the same plan and workspace, then the
    form's entry point of _SINK_SYMBOLS, which takes the descales, the cache's dtype code and the window (0 = none) in every form.
    ``family`` "tree" (flash_attention_tree*: ``tree_mask``, a dense int64 ``[B, Sq]`` tensor on Q's device, read by the kernel as
    bit patterns): the plan of flash_attention_tree_plan, then the entry point of _TREE_SYMBOLS -- the sinks one of decode without
    is_causal, with ``sinks`` (or NULL) and the mask."""
    import torch
    paged, ragged = block_table is not None, cu_seqlens_q is not None
    tree = family == "tree"
    symbols = _SPLIT_SYMBOLS["decode" if tree else family, paged, ragged]
    name = _TREE_SYMBOLS[paged] if tree else symbols[0][0]      # in the error texts: the un-windowed front's
    kv, layout = ("K_pool, V_pool", "[P, Hkv, page, d]") if paged else ("K, V", "[B, Hkv, capacity, d]")
    if ragged:
        Q = _token_view(Q, "Q")
    # (a contiguous cache is checked against the batch, so cu_seqlens_q comes before the tensors; with a table it comes after them)
    B = _cu_seqlens(cu_seqlens_q, Q) if ragged and not paged and Q.is_cuda else None
    fp8 = _decode_inputs(name, kv, layout, Q, K, V, k_descale, v_descale, table=block_table, batch=B)
    B = _cu_seqlens(cu_seqlens_q, Q) if ragged else Q.shape[0]
    capacity, tables, geometry = _cache_geometry(K, block_table, B)
    if ragged and O is not None:
        O = _token_view(O, "O")
    window = _window(window)
    both = family == "extend" or bool(window) or sinks is not None or tree
    _, H, Sq, d = Q.shape
    if sinks is not None and (getattr(sinks, "dtype", None) != torch.float32 or not sinks.is_cuda or sinks.device != Q.device
                              or tuple(sinks.shape) != (H,) or not sinks.is_contiguous()):
        raise ValueError("sinks must be a dense fp32 tensor [H] on the device of Q")
    if tree and (getattr(tree_mask, "dtype", None) != torch.int64 or not tree_mask.is_cuda or tree_mask.device != Q.device
                 or tuple(tree_mask.shape) != (B, Sq) or not tree_mask.is_contiguous()):
        raise ValueError("tree_mask must be a dense int64 tensor [B, Sq] on the device of Q")
    new = torch.zeros if ragged else torch.empty      # ragged: rows no sequence owns are not written
    Hkv = K.shape[1]
    _check_kv_lens(kv_lens, B)
    if scale is None:
        scale = 1.0 / float(d) ** 0.5
    odt = _dtype_code(out_dtype or (O.dtype if O is not None else _default_out_dtype(Q.dtype)))
    ns = _split_plan(family, ragged, B, H, Hkv, Sq, capacity, d, odt, num_splits, window).num_splits
    need = decode_workspace_size(1 if ragged else B, H, Sq, d, ns)
    with torch.cuda.device(Q.device):
        s = stream if stream is not None else torch.cuda.current_stream()
        # the workspace (like an O or LSE allocated here) belongs to the stream the kernels run on: see flash_attention_backward
        with torch.cuda.stream(s):
            if O is None:
                O = new((Sq, H, d), dtype=out_dtype or _default_out_dtype(Q.dtype), device=Q.device).unsqueeze(0).transpose(1, 2) if ragged \
                    else new((B, H, Sq, d), dtype=out_dtype or _default_out_dtype(Q.dtype), device=Q.device)
            elif O.shape != Q.shape or not O.is_cuda:
                raise ValueError("O must be a device tensor shaped like Q")
            lse = new((H, Sq) if ragged else (B, H, Sq), dtype=torch.float32, device=Q.device) if return_lse else None
            if workspace is None and need:
                workspace = torch.empty(need, dtype=torch.uint8, device=Q.device)
        if need and (not workspace.is_cuda or workspace.numel() * workspace.element_size() < need):
            raise ValueError(f"workspace must be a device tensor of at least {need} bytes")
        st = [_strides(t) for t in (Q, K, V, O)]
        ptr = lambda t: t.data_ptr() if t is not None else None
        ptrs = (Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), ptr(lse), *((ptr(cu_seqlens_q),) if ragged else ()), ptr(kv_lens),
                *map(ptr, tables))
        if fp8 or both:
            ptrs += (ptr(k_descale), ptr(v_descale))
        if sinks is not None or tree:
            ptrs += (ptr(sinks),)
        if tree:
            ptrs += (tree_mask.data_ptr(),)
        dtypes = (_dtype_code(Q.dtype), _dtype_code(K.dtype)) if fp8 or both else (_dtype_code(Q.dtype),)
        launch = getattr(lib(), name if tree else _SINK_SYMBOLS[family, paged, ragged] if sinks is not None else symbols[bool(window)][fp8])
        rc = launch(*ptrs, workspace.data_ptr() if need else None, B, H, Hkv, Sq, *geometry, d, float(scale),
                    *(() if tree else (bool(is_causal),)), *dtypes, _dtype_code(O.dtype), ns,
                    *((window,) if window or sinks is not None or tree else ()), *[ctypes.byref(x) for x in st], _stream_ptr(s))
    _check(rc)
    if ragged:
        O = O.transpose(1, 2).squeeze(0)      # back to [T, H, d]
    return (O, lse) if return_lse else O


def flash_attention_decode(Q, K, V, kv_lens=None, scale=None, is_causal=False, out_dtype=None, num_splits=0, return_lse=False,
                           O=None, workspace=None, stream=None, k_descale=None, v_descale=None, window=None, sinks=None):
    """Split-KV decode: Q ``[B, H, Sq, d]`` with 1 <= Sq <= FA_DECODE_MAX_Q new rows per sequence against a K/V cache
    ``[B, Hkv, capacity, d]`` (bf16, d = 64 or 128, Hkv dividing H; query head h reads K/V head ``h // (H // Hkv)``).

    ``kv_lens``: int32 device tensor ``[B]``, the valid keys of each sequence, read by the kernel (the call never synchronises; a
    captured graph sees the lengths of the moment), or None = the capacity.  Keys at and beyond the length may hold anything.
    ``is_causal`` is BOTTOM-RIGHT aligned: the Sq rows are the last rows of the sequence, row i sees keys
    ``k <= kv_lens[b] - Sq + i`` (and at least key 0) -- unlike ``flash_attention``, whose mask is top-left aligned.
    ``num_splits``: 0 = the library's choice (``decode_plan``), > 0 forced.  ``workspace`` (uint8 device tensor of
    ``decode_workspace_size`` bytes), when not given, is allocated with torch on the call's stream, like an ``O`` allocated here.
    Strided views are accepted (last dimension contiguous).  Returns O, or ``(O, LSE)`` with ``return_lse=True`` (fp32 [B, H, Sq],
    natural log).  Asynchronous on ``stream`` (default: torch's current stream).  No CPU fallback.

    fp8 cache: K and V of ``torch.float8_e4m3fn`` under a bf16 Q, with ``k_descale`` / ``v_descale``: fp32 device tensors ``[Hkv]``
    (None = 1), read by the kernel like ``kv_lens``.  The logical cache is ``K.float() * k_descale[kvh]``, ``V.float() *
    v_descale[kvh]``; the conversion is exact and everything else is as for bf16 (``decode_plan`` does not depend on the cache type).

    ``window``: None or 0 = none; W > 0 = a sliding window: row i sees at most the last W keys up to and including its own position,
    ``max(limC_i - W, 0) <= k`` with ``limC_i = max(kv_lens[b] - Sq + i + 1, 1)``, below ``limC_i`` with ``is_causal`` and below
    ``kv_lens[b]`` without (flash-attn's ``window_size=(W - 1, 0)`` / ``(W - 1, -1)``).  Keys below row 0's left edge are not read
    and may hold anything; ``decode_plan(..., window=W)`` plans from the window's tiles.  A negative window raises ValueError.

    ``sinks``: None, or ATTENTION SINKS: a dense fp32 device tensor ``[H]``, one logit per query head (natural-log units, not
    multiplied by ``scale``), read by the kernel like ``kv_lens``.  Every row's softmax gains one key of that score and value 0,
    whatever the mask, the window and the length, once per row: ``O = sum_k exp(s_k) v_k / (sum_k exp(s_k) + exp(sink_h))`` and the
    returned LSE includes the sink.  ``-inf`` is no sink (the call's bits without ``sinks``); any finite value gives finite results;
    ``+inf`` / NaN are the caller's error.  The plan and the workspace do not depend on it.  Anything but such a tensor raises
    ValueError.  Every decode and extend front takes it, with this meaning."""
    return _split_front("decode", Q, K, V, None, None, kv_lens, scale, is_causal, out_dtype, num_splits, return_lse, O, workspace, stream,
                        k_descale, v_descale, window, sinks)


def flash_attention_decode_paged(Q, K_pool, V_pool, block_table, kv_lens=None, scale=None, is_causal=False, out_dtype=None,
                                 num_splits=0, return_lse=False, O=None, workspace=None, stream=None, k_descale=None,
                                 v_descale=None, window=None, sinks=None):
    """``flash_attention_decode`` against PAGED K/V caches: Q ``[B, H, Sq, d]``, pools ``[P, Hkv, page, d]`` (bf16, d = 64 or 128,
    page a power of two >= 16; strided views accepted, so a ``[P, page, Hkv, d]`` pool is ``pool.transpose(1, 2)``) and
    ``block_table``: int32 device tensor ``[B, max_pages]`` with a contiguous last dimension (a row slice of a wider table is
    fine).  Key k of sequence b is row ``k % page`` of page ``block_table[b, k // page]``; sequences may share pages.

    The capacity ``max_pages * page`` plays the part of ``flash_attention_decode``'s cache capacity: ``kv_lens`` (int32 device
    tensor ``[B]``, or None = the capacity) is clamped into [1, capacity], and ``decode_plan`` / ``decode_workspace_size`` called
    with ``Sk = max_pages * page`` describe this call.  Table entries and lengths are read by the kernel (the call never
    synchronises; a captured graph sees the table of the moment): only the entries of pages that hold a key below the length,
    each clamped into [0, P).  Rows beyond the length and pages not named may hold anything.  Mask, ``num_splits``, ``workspace``,
    ``O``, ``return_lse`` and ``stream`` as for ``flash_attention_decode``; the result is that call's on a contiguous copy of the
    same pages, bit for bit.  fp8 pools (``torch.float8_e4m3fn`` under a bf16 Q) with ``k_descale`` / ``v_descale`` as for
    ``flash_attention_decode``.  ``window`` as there: a page whose keys all lie below row 0's left edge is not read and neither is
    its table entry, which may be any int32 (the engine may have freed the page).  ``sinks`` as there.  No CPU fallback."""
    return _split_front("decode", Q, K_pool, V_pool, block_table, None, kv_lens, scale, is_causal, out_dtype, num_splits, return_lse, O,
                        workspace, stream, k_descale, v_descale, window, sinks)


def flash_attention_extend(Q, K, V, kv_lens=None, scale=None, is_causal=False, out_dtype=None, num_splits=0, return_lse=False,
                           O=None, workspace=None, stream=None, k_descale=None, v_descale=None, sinks=None):
    """Chunked prefill against a decode cache: Q ``[B, H, Sq, d]`` with 1 <= Sq <= capacity new rows per sequence against the K/V
    cache ``[B, Hkv, capacity, d]`` that ``flash_attention_decode`` reads (bf16, or ``torch.float8_e4m3fn`` under a bf16 Q with
    ``k_descale`` / ``v_descale``; d = 64 or 128, Hkv dividing H).  Everything is ``flash_attention_decode``'s -- ``kv_lens`` (which
    already counts the new rows: ``kv_lens += Sq; kv_cache_append; flash_attention_extend``), the bottom-right ``is_causal``,
    ``num_splits``, ``workspace`` (``decode_workspace_size`` bytes for ``extend_plan``'s split count), ``O``, ``return_lse``,
    ``stream`` -- without the cap on Sq and without ``window`` (that is ``flash_attention_extend_window``).  For Sq <= 16 the result is
    that call's, bit for bit, under the same forced ``num_splits``.  ``sinks``: attention sinks, as in ``flash_attention_decode``.
    No CPU fallback."""
    return _split_front("extend", Q, K, V, None, None, kv_lens, scale, is_causal, out_dtype, num_splits, return_lse, O, workspace, stream,
                        k_descale, v_descale, sinks=sinks)


def flash_attention_extend_window(Q, K, V, kv_lens=None, window=None, **kw):
    """``flash_attention_extend`` with a SLIDING WINDOW: the same arguments plus ``window``.  W > 0: decode's rule with this call's Sq --
    row i sees ``max(limC_i - W, 0) <= k`` with ``limC_i = max(kv_lens[b] - Sq + i + 1, 1)``, below ``limC_i`` with ``is_causal`` and
    below ``kv_lens[b]`` without.  Keys below row 0's left edge are not read and may hold anything.  A row block walks only the tiles from
    its own rows' left edge on, so a long windowed chunk reads about W + rows keys per block, not the whole prefix
    (``extend_plan(..., window=W)``).  None or 0: ``flash_attention_extend`` itself, the same launches and bits.  For Sq <= 16 the result
    is ``flash_attention_decode(window=W)``'s, bit for bit, under the same forced ``num_splits``.  A negative window raises ValueError.
    No CPU fallback."""
    return _split_front("extend", Q, K, V, None, None, kv_lens, window=window, **kw)


def flash_attention_extend_paged(Q, K_pool, V_pool, block_table, kv_lens=None, scale=None, is_causal=False, out_dtype=None,
                                 num_splits=0, return_lse=False, O=None, workspace=None, stream=None, k_descale=None,
                                 v_descale=None, sinks=None):
    """``flash_attention_extend`` against PAGED K/V caches: the pools ``[P, Hkv, page, d]`` and the int32 ``block_table``
    ``[B, max_pages]`` of ``flash_attention_decode_paged``, with that call's rules for the table, the lengths and the capacity
    ``max_pages * page`` (``extend_plan`` is asked with ``Sk = max_pages * page``).  The result is ``flash_attention_extend``'s on a
    contiguous copy of the same pages, bit for bit.  No ``window`` (``flash_attention_extend_paged_window``).  No CPU fallback."""
    return _split_front("extend", Q, K_pool, V_pool, block_table, None, kv_lens, scale, is_causal, out_dtype, num_splits, return_lse, O,
                        workspace, stream, k_descale, v_descale, sinks=sinks)


def flash_attention_extend_paged_window(Q, K_pool, V_pool, block_table, kv_lens=None, window=None, **kw):
    """``flash_attention_extend_paged`` with a sliding window, as ``flash_attention_extend_window``: a page wholly below row 0's left
    edge is not read and neither is its table entry, which may be any int32.  The result is ``flash_attention_extend_window``'s on a
    contiguous copy of the same pages, bit for bit.  No CPU fallback."""
    return _split_front("extend", Q, K_pool, V_pool, block_table, None, kv_lens, window=window, **kw)


def flash_attention_extend_varlen(Q, K, V, cu_seqlens_q, kv_lens=None, scale=None, is_causal=False, out_dtype=None, num_splits=0,
                                  return_lse=False, O=None, workspace=None, stream=None, k_descale=None, v_descale=None, sinks=None):
    """RAGGED chunked prefill against a decode cache: one call for a mixed batch -- decoding sequences, chunks of a prefill, idle
    slots -- on token-major tensors.  Q ``[T, H, d]`` bf16 (strided views accepted, last dimension contiguous), packed by token;
    ``cu_seqlens_q``: int32 device tensor ``[B + 1]``, sequence b owns the rows ``cu[b] .. cu[b + 1] - 1`` (each pair clamped into
    [0, T]; a sequence without rows is an idle slot), read by the kernel like ``kv_lens``; K, V: the cache ``[B, Hkv, capacity, d]``
    of ``flash_attention_extend``, bf16 or ``torch.float8_e4m3fn`` with ``k_descale`` / ``v_descale``.  T is a bound (the allocation):
    rows beyond ``cu[-1]`` are not written.

    Per sequence everything is ``flash_attention_extend``'s with that sequence's row count: ``kv_lens[b]`` already counts the new
    rows, the bottom-right ``is_causal``, the tiles and splits -- the O and LSE of a sequence are, bit for bit, those of
    ``flash_attention_extend`` on that sequence alone under the same forced ``num_splits``.  ``num_splits`` 0 = the library's choice
    (``extend_varlen_plan``); ``workspace``: ``decode_workspace_size(1, H, T, d, ns)`` bytes.  Returns O ``[T, H, d]`` or, with
    ``return_lse``, ``(O, LSE)`` with the LSE fp32 ``[H, T]``; an O or LSE allocated here is zero-filled.  No ``window``
    (``flash_attention_extend_varlen_window``).  No CPU fallback."""
    return _split_front("extend", Q, K, V, None, cu_seqlens_q, kv_lens, scale, is_causal, out_dtype, num_splits, return_lse, O, workspace,
                        stream, k_descale, v_descale, sinks=sinks)


def flash_attention_extend_varlen_window(Q, K, V, cu_seqlens_q, kv_lens=None, window=None, **kw):
    """``flash_attention_extend_varlen`` with a sliding window: ``flash_attention_extend_window``'s rule per sequence with its own row
    count (``extend_varlen_plan(..., window=W)``); None or 0: ``flash_attention_extend_varlen`` itself.  The O and LSE of a sequence are,
    bit for bit, those of ``flash_attention_extend_window`` on that sequence alone under the same forced ``num_splits``.  No CPU
    fallback."""
    return _split_front("extend", Q, K, V, None, cu_seqlens_q, kv_lens, window=window, **kw)


def flash_attention_extend_paged_varlen(Q, K_pool, V_pool, block_table, cu_seqlens_q, kv_lens=None, scale=None, is_causal=False,
                                        out_dtype=None, num_splits=0, return_lse=False, O=None, workspace=None, stream=None,
                                        k_descale=None, v_descale=None, sinks=None):
    """``flash_attention_extend_varlen`` against PAGED K/V caches: the pools ``[P, Hkv, page, d]`` and the int32 ``block_table``
    ``[B, max_pages]`` of ``flash_attention_extend_paged`` (``extend_varlen_plan`` is asked with ``Sk = max_pages * page``).  The
    table row and the length of a sequence without rows are not read.  The result is ``flash_attention_extend_varlen``'s on a
    contiguous copy of the same pages, bit for bit.  No ``window`` (``flash_attention_extend_paged_varlen_window``).  No CPU fallback."""
    return _split_front("extend", Q, K_pool, V_pool, block_table, cu_seqlens_q, kv_lens, scale, is_causal, out_dtype, num_splits,
                        return_lse, O, workspace, stream, k_descale, v_descale, sinks=sinks)


def flash_attention_extend_paged_varlen_window(Q, K_pool, V_pool, block_table, cu_seqlens_q, kv_lens=None, window=None, **kw):
    """``flash_attention_extend_paged_varlen`` with a sliding window, as ``flash_attention_extend_varlen_window``; pages below a
    sequence's window as in ``flash_attention_extend_paged_window``.  No CPU fallback."""
    return _split_front("extend", Q, K_pool, V_pool, block_table, cu_seqlens_q, kv_lens, window=window, **kw)


def flash_attention_tree(Q, K, V, tree_mask, kv_lens=None, scale=None, out_dtype=None, num_splits=0, return_lse=False, k_descale=None,
                         v_descale=None, window=0, sinks=None, stream=None):
    """TREE-MASKED VERIFICATION of a speculative draft: Q ``[B, H, Sq, d]`` holds the 1 <= Sq <= FA_TREE_MAX_Q draft nodes of the
    step, already appended to the cache ``[B, Hkv, capacity, d]`` (bf16 or fp8 with descales) and counted by ``kv_lens``: node j is
    key ``base + j`` with ``base = kv_lens[b] - Sq``, node i is query row i of every head.

    ``tree_mask``: dense ``torch.int64`` device tensor ``[B, Sq]``, read by the kernel as bit patterns (no host synchronisation; a
    replayed graph sees the words of the moment): bit j of word (b, i) set = row i sees node j.  Row i sees key k iff the causal
    call (``flash_attention_decode(..., is_causal=True)`` with the same ``window``) shows it AND (``k < base``, or bit ``k - base``
    is set, or k is the row's own key).  So the own key is always visible, bits above i and at or beyond Sq are ignored, and an
    all-ones word or a chain is the causal call itself, bit for bit (Sq <= 16: ``flash_attention_decode``; above:
    ``flash_attention_extend``).  ``window`` counts cache positions, not tree depth.  ``sinks``, ``num_splits``, ``out_dtype``,
    ``return_lse``, the descales and ``stream`` as for ``flash_attention_decode``; ``tree_plan`` describes the launches.
    ``tree_mask_from_parents`` builds the words from parent indices.  No CPU fallback."""
    return _split_front("tree", Q, K, V, None, None, kv_lens, scale, True, out_dtype, num_splits, return_lse, None, None, stream,
                        k_descale, v_descale, window, sinks, tree_mask)


def flash_attention_tree_paged(Q, K_pool, V_pool, block_table, tree_mask, kv_lens=None, scale=None, out_dtype=None, num_splits=0,
                               return_lse=False, k_descale=None, v_descale=None, window=0, sinks=None, stream=None):
    """``flash_attention_tree`` against PAGED caches (pools ``[P, Hkv, page, d]`` and ``block_table`` as for
    ``flash_attention_decode_paged``): the result is that call's on a contiguous copy of the same pages, bit for bit."""
    return _split_front("tree", Q, K_pool, V_pool, block_table, None, kv_lens, scale, True, out_dtype, num_splits, return_lse, None, None,
                        stream, k_descale, v_descale, window, sinks, tree_mask)


def _cascade_splits(num_splits):
    """``num_splits`` of the cascade fronts as the C ABI's pair: ``(shared, unique)``, 0 = the library's choice"""
    try:
        ns_s, ns_u = (int(n) for n in num_splits)
    except (TypeError, ValueError):
        raise ValueError("num_splits must be a pair (shared, unique); 0 = the library's choice") from None
    return ns_s, ns_u


def cascade_plan(B, H, Hkv, Sq, Ls, Sk, d, o_dtype=FA_DTYPE_BF16, num_splits=(0, 0)):
    """What a flash_attention_cascade_decode call launches (fa_cascade_plan as a dict): ``shared`` and ``unique`` are the plans of the two
    split launches (``Ls``, ``Sk``: the capacities of the shared part and of the suffixes), ``num_splits`` their sum -- what
    ``decode_workspace_size(B, H, Sq, d, num_splits)`` is asked with.  ``num_splits``: the pair (shared, unique), 0 = the library's choice."""
    p = FaCascadePlan()
    ns_s, ns_u = _cascade_splits(num_splits)
    _check(lib().flash_attention_cascade_plan(B, H, Hkv, Sq, Ls, Sk, d, o_dtype, ns_s, ns_u, ctypes.byref(p)))
    return {"shared": _plan_dict(p.shared), "unique": _plan_dict(p.unique), "num_splits": p.num_splits}


def _cascade_front(Q, K_shared, V_shared, K, V, shared_table, block_table, shared_len, kv_lens, scale, is_causal, out_dtype, num_splits,
                   return_lse, O, workspace, stream, k_descale, v_descale, sinks):
    """Both cascade fronts: the checks of the decode fronts on the suffix caches, the same on the shared ones, the plan and the
    workspace as ``_split_front`` allocates it, then the entry point of _CASCADE_SYMBOLS."""
    import torch
    paged = block_table is not None
    name = _CASCADE_SYMBOLS[paged]
    kv, layout = ("K_pool, V_pool", "[P, Hkv, page, d]") if paged else ("K, V", "[B, Hkv, capacity, d]")
    fp8 = _decode_inputs(name, kv, layout, Q, K, V, k_descale, v_descale, table=block_table)
    B, H, Sq, d = Q.shape
    Hkv = K.shape[1]
    if paged:
        t = shared_table
        if not getattr(t, "is_cuda", False) or t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < 1 or not t.is_contiguous() \
                or t.device != Q.device:
            raise ValueError("shared_table must be a dense int32 device tensor [max_shared_pages] on the device of Q")
        shared_capacity, shared_geometry = t.shape[0] * K.shape[2], (t.shape[0],)
    else:
        if not (getattr(K_shared, "is_cuda", False) and getattr(V_shared, "is_cuda", False)):
            raise RuntimeError(f"{name} needs device tensors (no CPU fallback)")
        if K_shared.dim() != 3 or K_shared.shape != V_shared.shape or K_shared.shape[0] != Hkv or K_shared.shape[2] != d \
                or K_shared.shape[1] < 1:
            raise ValueError("K_shared, V_shared must be [Hkv, shared capacity, d] with the Hkv and d of K, V")
        if not (K_shared.dtype == V_shared.dtype == K.dtype):
            raise TypeError("K_shared, V_shared, K, V must share a dtype")
        shared_capacity, shared_geometry = K_shared.shape[1], (K_shared.shape[1],)
    capacity, tables, geometry = _cache_geometry(K, block_table, B)
    if shared_len is not None and (not getattr(shared_len, "is_cuda", False) or shared_len.dtype != torch.int32 or shared_len.shape != (1,)
                                   or shared_len.device != Q.device):
        raise ValueError("shared_len must be an int32 device tensor [1] on the device of Q")
    if sinks is not None and (getattr(sinks, "dtype", None) != torch.float32 or not sinks.is_cuda or sinks.device != Q.device
                              or tuple(sinks.shape) != (H,) or not sinks.is_contiguous()):
        raise ValueError("sinks must be a dense fp32 tensor [H] on the device of Q")
    _check_kv_lens(kv_lens, B)
    if scale is None:
        scale = 1.0 / float(d) ** 0.5
    odt = _dtype_code(out_dtype or (O.dtype if O is not None else _default_out_dtype(Q.dtype)))
    ns_s, ns_u = _cascade_splits(num_splits)
    p = FaCascadePlan()
    _check(lib().flash_attention_cascade_plan(B, H, Hkv, Sq, shared_capacity, capacity, d, odt, ns_s, ns_u, ctypes.byref(p)))
    need = decode_workspace_size(B, H, Sq, d, p.num_splits)
    with torch.cuda.device(Q.device):
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            if O is None:
                O = torch.empty((B, H, Sq, d), dtype=out_dtype or _default_out_dtype(Q.dtype), device=Q.device)
            elif O.shape != Q.shape or not O.is_cuda:
                raise ValueError("O must be a device tensor shaped like Q")
            lse = torch.empty((B, H, Sq), dtype=torch.float32, device=Q.device) if return_lse else None
            if workspace is None:
                workspace = torch.empty(need, dtype=torch.uint8, device=Q.device)
        if not workspace.is_cuda or workspace.numel() * workspace.element_size() < need:
            raise ValueError(f"workspace must be a device tensor of at least {need} bytes")
        ptr = lambda t: t.data_ptr() if t is not None else None
        caches = (K, V) if paged else (K_shared, V_shared, K, V)
        st = [_strides(t.unsqueeze(0)) if t.dim() == 3 else _strides(t) for t in (Q, *caches, O)]
        rc = getattr(lib(), name)(Q.data_ptr(), *(t.data_ptr() for t in caches), O.data_ptr(), ptr(lse), ptr(shared_len), ptr(kv_lens),
                                  *((shared_table.data_ptr(), block_table.data_ptr()) if paged else ()), ptr(k_descale), ptr(v_descale),
                                  ptr(sinks), workspace.data_ptr(), B, H, Hkv, Sq,
                                  *((geometry[0], geometry[1], *shared_geometry, *geometry[2:]) if paged else (*shared_geometry, *geometry)),
                                  d, float(scale), bool(is_causal), _dtype_code(Q.dtype), _dtype_code(K.dtype), _dtype_code(O.dtype),
                                  p.shared.num_splits, p.unique.num_splits, *[ctypes.byref(x) for x in st], _stream_ptr(s))
    _check(rc)
    return (O, lse) if return_lse else O


def flash_attention_cascade_decode(Q, K_shared, V_shared, K, V, shared_len=None, kv_lens=None, scale=None, is_causal=False,
                                   out_dtype=None, num_splits=(0, 0), return_lse=False, O=None, workspace=None, stream=None,
                                   k_descale=None, v_descale=None, sinks=None):
    """SHARED-PREFIX (cascade) decode: the logical cache of sequence b is ``[K_shared[:, :ls] ; K[b, :, :kv_lens[b]]]`` -- one prefix
    ``[Hkv, shared capacity, d]`` that every sequence sees in full, read once per row block of the whole batch, then the sequence's own
    suffix ``[B, Hkv, capacity, d]``.  Q ``[B, H, Sq, d]``, 1 <= Sq <= FA_DECODE_MAX_Q, is the last Sq rows of that logical sequence.

    ``shared_len``: int32 device tensor ``[1]``, the valid shared keys, clamped into [1, shared capacity] on the device (None = the
    capacity); ``kv_lens`` as in ``flash_attention_decode``, of the suffixes.  There is no mask on the shared part; of its suffix a row
    sees what ``flash_attention_decode`` shows it on the suffix alone (``is_causal``: bottom-right, at least key 0), so whenever
    ``kv_lens[b] >= Sq`` the result is ``flash_attention_decode(is_causal=...)`` on the concatenated cache.  The LSE covers both parts.
    fp8 caches (all four tensors ``torch.float8_e4m3fn`` under a bf16 Q) take ONE ``k_descale`` / ``v_descale`` pair for both parts;
    ``sinks`` as in ``flash_attention_decode``.  ``num_splits``: the pair (shared, unique), 0 = the library's choice (``cascade_plan``);
    unique >= 2 when forced.  ``workspace``: ``decode_workspace_size(B, H, Sq, d, cascade_plan(...)["num_splits"])`` bytes, always
    needed, allocated on the call's stream when not given.  Three launches, asynchronous, graph-capturable.  No window.  No CPU fallback."""
    return _cascade_front(Q, K_shared, V_shared, K, V, None, None, shared_len, kv_lens, scale, is_causal, out_dtype, num_splits, return_lse,
                          O, workspace, stream, k_descale, v_descale, sinks)


def flash_attention_cascade_decode_paged(Q, K_pool, V_pool, shared_table, block_table, shared_len=None, kv_lens=None, scale=None,
                                         is_causal=False, out_dtype=None, num_splits=(0, 0), return_lse=False, O=None, workspace=None,
                                         stream=None, k_descale=None, v_descale=None, sinks=None):
    """``flash_attention_cascade_decode`` against PAGED caches: one pool pair ``[P, Hkv, page, d]`` serves both parts.
    ``shared_table``: int32 device tensor ``[max_shared_pages]``, the shared part's pages in order; ``block_table`` ``[B, max_pages]``
    holds the SUFFIX pages (an engine passes its table offset by the shared pages; the tail of a prompt that does not fill a page lives
    in the suffix).  ``shared_len`` is clamped into [1, max_shared_pages * page].  Entries are read and clamped by the kernel as in
    ``flash_attention_decode_paged``; the result is the contiguous call's on gathered copies under the same ``num_splits``, bit for bit."""
    return _cascade_front(Q, None, None, K_pool, V_pool, shared_table, block_table, shared_len, kv_lens, scale, is_causal, out_dtype,
                          num_splits, return_lse, O, workspace, stream, k_descale, v_descale, sinks)


# ---- MLA decode: one latent cache read as K (576 columns) and as V (the first 512) ----
MLA_D_LATENT, MLA_D_ROPE = 512, 64
_MLA_SYMBOLS = {False: "flash_attention_mla_decode", True: "flash_attention_mla_decode_paged"}


def mla_decode_plan(B, H, Sq, Sk, o_dtype=FA_DTYPE_BF16, num_splits=0):
    """What a flash_attention_mla_decode call launches (fa_decode_plan as a dict; ``Sk`` the capacity): row blocks of 64 packed rows
    ``h * Sq + i``, ``grid = B * row_blocks * num_splits``; ``num_splits`` 0 = the library's choice (a rule that is not measured).
    The workspace is ``decode_workspace_size(B, H, Sq, 512, num_splits)``."""
    p = FaDecodePlan()
    _check(lib().flash_attention_mla_decode_plan(B, H, Sq, Sk, MLA_D_LATENT, MLA_D_ROPE, o_dtype, num_splits, ctypes.byref(p)))
    return _plan_dict(p)


def _mla_front(Q, KV, block_table, kv_lens, scale, is_causal, out_dtype, num_splits, return_lse, O, workspace, stream):
    """Both MLA fronts: the checks of the tensors (with the decode fronts' helpers for the table, the lengths and the workspace), the plan
    and the workspace for the capacity, then the entry point of _MLA_SYMBOLS."""
    import torch
    paged = block_table is not None
    name = _MLA_SYMBOLS[paged]
    if not (Q.is_cuda and KV.is_cuda and (not paged or block_table.is_cuda)):
        raise RuntimeError(f"{name} needs device tensors (no CPU fallback)")
    D = MLA_D_LATENT + MLA_D_ROPE
    if Q.dim() != 4 or KV.dim() != 3 or (not paged and Q.shape[0] != KV.shape[0]) or Q.shape[3] != D or KV.shape[2] != D:
        raise ValueError(f"Q must be [B, H, Sq, {D}] and {'KV_pool [P, page' if paged else 'KV [B, capacity'}, {D}]")
    if Q.dtype != KV.dtype:
        raise TypeError("Q, KV must share a dtype")
    if KV.stride(2) != 1:
        raise ValueError("last dimension must be contiguous")
    B, H, Sq, _ = Q.shape
    # the cache as the [*, 1, rows, 576] tensor the decode helpers describe: one K/V "head"
    capacity, tables, geometry = _cache_geometry(KV.unsqueeze(1), block_table, B)
    _check_kv_lens(kv_lens, B)
    if scale is None:
        scale = float(D) ** -0.5
    odt = _dtype_code(out_dtype or (O.dtype if O is not None else _default_out_dtype(Q.dtype)))
    ns = mla_decode_plan(B, H, Sq, capacity, odt, num_splits)["num_splits"]
    need = decode_workspace_size(B, H, Sq, MLA_D_LATENT, ns)
    with torch.cuda.device(Q.device):
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            if O is None:
                O = torch.empty((B, H, Sq, MLA_D_LATENT), dtype=out_dtype or _default_out_dtype(Q.dtype), device=Q.device)
            elif tuple(O.shape) != (B, H, Sq, MLA_D_LATENT) or not O.is_cuda:
                raise ValueError(f"O must be a device tensor [B, H, Sq, {MLA_D_LATENT}]")
            lse = torch.empty((B, H, Sq), dtype=torch.float32, device=Q.device) if return_lse else None
            if workspace is None and need:
                workspace = torch.empty(need, dtype=torch.uint8, device=Q.device)
        if need and (not workspace.is_cuda or workspace.numel() * workspace.element_size() < need):
            raise ValueError(f"workspace must be a device tensor of at least {need} bytes")
        sQ, sO = _strides(Q), _strides(O)
        sKV = FaStrides(KV.stride(0), 0, KV.stride(1))
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = getattr(lib(), name)(Q.data_ptr(), KV.data_ptr(), O.data_ptr(), ptr(lse), ptr(kv_lens), *map(ptr, tables),
                                  workspace.data_ptr() if need else None, B, H, Sq, *geometry, MLA_D_LATENT, MLA_D_ROPE, float(scale),
                                  bool(is_causal), _dtype_code(Q.dtype), _dtype_code(O.dtype), ns,
                                  ctypes.byref(sQ), ctypes.byref(sKV), ctypes.byref(sO), _stream_ptr(s))
    _check(rc)
    return (O, lse) if return_lse else O


def flash_attention_mla_decode(Q, KV, kv_lens=None, scale=None, is_causal=False, out_dtype=None, num_splits=0, return_lse=False,
                               O=None, workspace=None, stream=None):
    """Decode for multi-head latent attention (DeepSeek-V2 / V3 / R1, Kimi-K2) in its absorbed form: Q ``[B, H, Sq, 576]`` (bf16; the
    absorbed ``q_nope @ W_UK`` in columns [0, 512), the rotated ``q_rope`` in [512, 576)), 1 <= Sq <= FA_DECODE_MAX_Q, against ONE
    latent cache ``KV [B, capacity, 576]`` shared by all heads: ``O = softmax(scale * Q KV^T) KV[:, :512]``, ``[B, H, Sq, 512]``.

    ``scale``: None = ``576 ** -0.5`` (FlashMLA's default, the full width of the score); a model passes its own softmax scale,
    ``mscale ** 2 / sqrt(192)`` -- the absorption does not change it.  ``kv_lens``, ``is_causal`` (bottom-right aligned),
    ``num_splits`` (0 = ``mla_decode_plan``'s choice), ``workspace`` (``decode_workspace_size(B, H, Sq, 512, ns)`` bytes), ``O``,
    ``return_lse`` and ``stream`` as for ``flash_attention_decode``; strided views are accepted (last dimension contiguous).
    The cache row is fetched once per 64 packed rows and serves both products.  No CPU fallback."""
    return _mla_front(Q, KV, None, kv_lens, scale, is_causal, out_dtype, num_splits, return_lse, O, workspace, stream)


def flash_attention_mla_decode_paged(Q, KV_pool, block_table, kv_lens=None, scale=None, is_causal=False, out_dtype=None, num_splits=0,
                                     return_lse=False, O=None, workspace=None, stream=None):
    """``flash_attention_mla_decode`` against a PAGED latent cache: ``KV_pool [P, page, 576]`` (page a power of two >= 16) and
    ``block_table`` int32 ``[B, max_pages]`` as in ``flash_attention_decode_paged``: entries and lengths are read and clamped by the
    kernel, pages no visible key lies in are not read.  ``scale`` None = ``576 ** -0.5``.  The result is the contiguous call's on a
    gathered copy under the same ``num_splits``, bit for bit."""
    return _mla_front(Q, KV_pool, block_table, kv_lens, scale, is_causal, out_dtype, num_splits, return_lse, O, workspace, stream)


def _tree_parents(parents):
    """the checks of a parent array: integers ``[B, Sq]``, Sq <= FA_TREE_MAX_Q, -1 for a root, else ``0 <= parent < index``"""
    import torch
    p = torch.as_tensor(parents)
    if p.dim() != 2 or p.shape[1] < 1 or p.shape[1] > FA_TREE_MAX_Q or p.dtype.is_floating_point or p.dtype == torch.bool:
        raise ValueError(f"parents must be integers [B, Sq] with 1 <= Sq <= {FA_TREE_MAX_Q}")
    p = p.long()
    if bool(((p < -1) | (p >= torch.arange(p.shape[1], device=p.device)[None, :])).any()):      # (a device tensor: one synchronisation)
        raise ValueError("parents must be -1 (a root) or the index of an earlier node")
    return p


def tree_mask_from_parents(parents):
    """The ``tree_mask`` words of a draft tree given as parent indices: ``parents`` ``[B, Sq]`` integers (a tensor on any device, or
    nested lists), -1 for a root, else ``parent < index`` (nodes in any topological order).  Returns ``torch.int64 [B, Sq]`` on the
    device of ``parents``: word i has the bits of node i's ancestors and its own (ancestor-closed)."""
    import torch
    p = _tree_parents(parents)
    w = torch.zeros_like(p)
    one = torch.ones((), dtype=torch.int64, device=p.device)
    for i in range(p.shape[1]):
        up = torch.gather(w, 1, p[:, i:i + 1].clamp(min=0))[:, 0]
        w[:, i] = torch.where(p[:, i] >= 0, up, torch.zeros_like(up)) | (one << i)
    return w


def tree_depths(parents):
    """Depth of every node of a draft tree (``parents`` as for ``tree_mask_from_parents``): ``torch.int32 [B, Sq]``, 0 for a root.
    Node i's position in ITS sequence is ``base + depth``: the result is what ``rope_cache_append(..., pos_offsets=)`` takes, which
    then rotates node i at ``base + depth`` and still stores it at slot ``base + i``."""
    import torch
    p = _tree_parents(parents)
    dep = torch.zeros_like(p)
    for i in range(p.shape[1]):
        up = torch.gather(dep, 1, p[:, i:i + 1].clamp(min=0))[:, 0]
        dep[:, i] = torch.where(p[:, i] >= 0, up + 1, torch.zeros_like(up))
    return dep.to(torch.int32)


def tree_path(parents, leaf):
    """The accepted path of a draft tree as ``kv_cache_accept`` takes it: ``parents`` as for ``tree_mask_from_parents``, ``leaf`` an
    integer tensor ``[B]``, the last accepted node of every sequence (clamped into the tree).  Returns ``(accept_idx, accept_lens)``,
    int32 ``[B, Sq]`` and ``[B]`` on the device of ``parents``: the nodes from the root down to ``leaf``, the tail padded with
    ``Sq - 1``, and their count ``depth(leaf) + 1``.  Torch ops only, a number of steps known from the shape.  A DEVICE tensor of
    parents is taken as it is -- nothing is read back to the host, so a captured graph may contain the call; entries that are not
    parents (>= their index, < -1) give some path inside the tree, never an index outside it.  Parents given on the host go through
    the check of ``tree_mask_from_parents``."""
    import torch
    if isinstance(parents, torch.Tensor) and parents.is_cuda:
        if parents.dim() != 2 or not 1 <= parents.shape[1] <= FA_TREE_MAX_Q or parents.dtype.is_floating_point or parents.dtype == torch.bool:
            raise ValueError(f"parents must be integers [B, Sq] with 1 <= Sq <= {FA_TREE_MAX_Q}")
        p = parents.long()
    else:
        p = _tree_parents(parents)
    B, Sq = p.shape
    leaf = torch.as_tensor(leaf, device=p.device)
    if leaf.shape != (B,) or leaf.dtype.is_floating_point or leaf.dtype == torch.bool:
        raise ValueError("leaf must be an integer tensor [B]")
    node = leaf.long().clamp(0, Sq - 1)
    up = torch.full((B, Sq), -1, dtype=torch.int64, device=p.device)      # up[:, k]: the k-th node from the leaf upwards, -1 past the root
    for k in range(Sq):
        up[:, k] = node
        nxt = torch.gather(p, 1, node.clamp(min=0)[:, None])[:, 0].clamp(-1, Sq - 1)
        node = torch.where(node >= 0, nxt, node)
    n = (up >= 0).sum(dim=1)
    at = n[:, None] - 1 - torch.arange(Sq, device=p.device)[None, :]      # root first: entry t is up[n - 1 - t]
    idx = torch.where(at >= 0, torch.gather(up, 1, at.clamp(min=0)), torch.full_like(up, Sq - 1))
    return idx.to(torch.int32), n.to(torch.int32)


def _accept_front(name, K, V, block_table, accept_idx, accept_lens, kv_lens, stream):
    """The kv_cache_accept* fronts: the cache checks of the append fronts without new rows, and the entry point of _ACCEPT_SYMBOLS"""
    import torch
    paged = block_table is not None
    kv, layout = ("K_pool, V_pool", "[P, Hkv, page, d]") if paged else ("K_cache, V_cache", "[B, Hkv, capacity, d]")
    if not (getattr(K, "is_cuda", False) and getattr(V, "is_cuda", False) and getattr(accept_idx, "is_cuda", False)
            and getattr(accept_lens, "is_cuda", False) and (not paged or block_table.is_cuda)):
        raise RuntimeError(f"{name} needs device tensors (no CPU fallback)")
    f8 = getattr(torch, "float8_e4m3fn", None)
    if K.dim() != 4 or K.shape != V.shape or K.dtype != V.dtype or K.device != V.device:
        raise ValueError(f"{kv} must be {layout} of one dtype on one device")
    if K.dtype != torch.bfloat16 and (f8 is None or K.dtype != f8):
        raise TypeError(f"{kv} must be bfloat16 or float8_e4m3fn")
    if accept_idx.dtype != torch.int32 or accept_idx.dim() != 2 or not accept_idx.is_contiguous() or accept_idx.device != K.device:
        raise ValueError("accept_idx must be a dense int32 device tensor [B, Sq] on the device of the caches")
    B, Sq = accept_idx.shape
    if not paged and K.shape[0] != B:
        raise ValueError(f"{kv} {layout}: the batch of accept_idx")
    if accept_lens.dtype != torch.int32 or accept_lens.shape != (B,) or not accept_lens.is_contiguous() or accept_lens.device != K.device:
        raise ValueError("accept_lens must be a dense int32 device tensor [B] on the device of the caches")
    capacity, tables, geometry = _cache_geometry(K, block_table, B)
    if Sq < 1 or Sq > FA_TREE_MAX_Q or Sq > capacity:
        raise ValueError(f"Sq = {Sq} draft nodes: must be 1 .. min(FA_TREE_MAX_Q, the capacity) ({min(FA_TREE_MAX_Q, capacity)})")
    _check_kv_lens(kv_lens, B)
    ptr = lambda t: t.data_ptr() if t is not None else None
    with torch.cuda.device(K.device):
        st = [_strides(K), _strides(V)]
        rc = getattr(lib(), _ACCEPT_SYMBOLS[paged])(
            K.data_ptr(), V.data_ptr(), ptr(kv_lens), *map(ptr, tables), accept_idx.data_ptr(), accept_lens.data_ptr(), B, K.shape[1], Sq,
            *geometry, K.shape[3], _dtype_code(K.dtype), *[ctypes.byref(x) for x in st], _stream_ptr(stream))
    _check(rc)


def kv_cache_accept(K_cache, V_cache, accept_idx, accept_lens, kv_lens=None, stream=None):
    """IN-CACHE ACCEPTANCE of a speculative step, in place; returns None.  The draft's Sq nodes lie at the cache positions
    ``base + 0 .. base + Sq - 1`` (``kv_lens`` still counts them: ``base = min(kv_lens[b], capacity) - Sq``); per sequence, for
    ``t = 0 .. n - 1`` in ascending order, K and V of every head at ``base + accept_idx[b, t]`` are copied to ``base + t``
    (``n = clamp(accept_lens[b], 0, Sq)``, indices clamped into the draft) -- a copy of bits, bf16 or float8_e4m3fn.  For the path
    of a topologically ordered tree (``tree_path``) row t becomes the draft's row ``accept_idx[b, t]``; with
    ``rope_cache_append(..., pos_offsets=tree_depths(parents))`` the cache then holds what a linear ``rope_cache_append`` of the
    accepted tokens writes, byte for byte.  Nothing else is written, ``kv_lens`` included: follow with
    ``kv_lens -= Sq - accept_lens``.  ``accept_idx`` int32 ``[B, Sq]``, ``accept_lens`` int32 ``[B]``, device tensors read by the
    kernel: no synchronisation, one graph for the whole step.  1 <= Sq <= FA_TREE_MAX_Q.  No CPU fallback."""
    _accept_front("kv_cache_accept", K_cache, V_cache, None, accept_idx, accept_lens, kv_lens, stream)


def kv_cache_accept_paged(K_pool, V_pool, block_table, accept_idx, accept_lens, kv_lens=None, stream=None):
    """``kv_cache_accept`` in the PAGED caches of ``kv_cache_append_paged``.  A move whose source or destination page entry is
    outside [0, P) is skipped, never clamped."""
    _accept_front("kv_cache_accept_paged", K_pool, V_pool, block_table, accept_idx, accept_lens, kv_lens, stream)


def _append_front(name, K_new, V_new, K, V, block_table, cu_seqlens_q, kv_lens, k_descale, v_descale, stream, rope=None, pos_offsets=None):
    """The kv_cache_append* and rope_cache_append* fronts (``name``: the front's, in the error texts): a ``block_table`` makes the call
    paged (K, V are then the pools) and ``cu_seqlens_q`` ragged (the new rows are then packed by token: Sq is the bound on the packed
    rows, not capped at the capacity, and the batch is cu_seqlens_q's).  The tensor checks of the decode fronts (``_decode_inputs``,
    the new rows in the place of Q), the bounds of Sq, and the entry point of _APPEND_SYMBOLS.  ``rope`` = (Q, Q_out, cos_sin,
    interleaved) makes it the fused call: Q, Q_out and the table are checked as well, the entry point is _ROPE_SYMBOLS' and the
    rotated queries are returned (ragged: ``[T, H, d]``).  ``pos_offsets`` (uniform fused calls only) makes it _ROPE_POS_SYMBOLS'."""
    import torch
    paged, ragged = block_table is not None, cu_seqlens_q is not None
    Q, Q_out, cos_sin, interleaved = rope or (None,) * 4
    kv, layout = ("K_pool, V_pool", "[P, Hkv, page, d]") if paged else ("K_cache, V_cache", "[B, Hkv, capacity, d]")
    if ragged:
        K_new, V_new = _token_view(K_new, "K_new"), _token_view(V_new, "V_new")
        if rope:
            Q = _token_view(Q, "Q")
            if Q_out is not None:
                Q_out = _token_view(Q_out, "Q_out")
    elif paged:      # (the uniform paged front checks its table first; the ragged one where the batch is known)
        _table_geometry(block_table, K_new.shape[0] if K_new.dim() == 4 else 0)
    if K_new.dim() != 4 or V_new.dim() != 4 or K_new.shape != V_new.shape or K_new.dtype != V_new.dtype or (K.dim() == 4 and K_new.shape[1] != K.shape[1]):
        raise ValueError(f"K_new, V_new must be {'[T, Hkv, d]' if ragged else '[B, Hkv, Sq, d]'} of one dtype, with the K/V heads of {kv} {layout}")
    if not V_new.is_cuda or (rope and not Q.is_cuda):
        raise RuntimeError(f"{name} needs device tensors (no CPU fallback)")
    B = _cu_seqlens(cu_seqlens_q, K_new) if ragged and K_new.is_cuda else None
    _decode_inputs(name, kv, layout, K_new, K, V, k_descale, v_descale, table=block_table, batch=B)
    _, Hkv, Sq, d = K_new.shape
    if rope and (Q.dim() != 4 or Q.dtype != K_new.dtype or Q.device != K_new.device
                 or (Q.shape[0], Q.shape[2], Q.shape[3]) != (K_new.shape[0], Sq, d) or Q.shape[1] < 1 or Q.shape[1] % Hkv):
        raise ValueError(f"Q must be {'[T, H, d]' if ragged else '[B, H, Sq, d]'} of the dtype and on the device of K_new, with Hkv dividing H")
    if not ragged:
        B = K_new.shape[0]
    capacity, tables, geometry = _cache_geometry(K, block_table, B)
    if Sq < 1 or (Sq > capacity and not ragged):
        raise ValueError(f"Sq = {Sq} new rows: must be 1 .. the capacity ({capacity})")
    _check_kv_lens(kv_lens, B)
    ptr = lambda t: t.data_ptr() if t is not None else None
    if not rope:
        with torch.cuda.device(K_new.device):
            st = [_strides(t) for t in (K_new, V_new, K, V)]
            rc = getattr(lib(), _APPEND_SYMBOLS[paged, ragged])(
                K_new.data_ptr(), V_new.data_ptr(), K.data_ptr(), V.data_ptr(), *((ptr(cu_seqlens_q),) if ragged else ()), ptr(kv_lens),
                *map(ptr, tables), ptr(k_descale), ptr(v_descale), B, Hkv, Sq, *geometry, d, _dtype_code(K_new.dtype), _dtype_code(K.dtype),
                *[ctypes.byref(x) for x in st], _stream_ptr(stream))
        _check(rc)
        return None
    t = cos_sin
    if getattr(t, "dtype", None) != torch.float32 or not t.is_cuda or t.device != Q.device or t.dim() != 2 or not t.is_contiguous():
        raise ValueError("cos_sin must be a dense fp32 tensor [max_pos, rot_dim] on the device of Q")
    max_pos, rot_dim = t.shape
    if rot_dim % 16 or not 16 <= rot_dim <= d or max_pos < capacity:
        raise ValueError(f"cos_sin [max_pos, rot_dim]: rot_dim a multiple of 16 in 16 .. d, max_pos at least the capacity ({capacity})")
    if Q_out is not None and (not getattr(Q_out, "is_cuda", False) or Q_out.shape != Q.shape or Q_out.dtype != Q.dtype or Q_out.device != Q.device):
        raise ValueError("Q_out must be a device tensor shaped like Q, of its dtype, on its device")
    po = pos_offsets
    if po is not None and (not getattr(po, "is_cuda", False) or po.dtype != torch.int32 or tuple(po.shape) != (B, Sq) or not po.is_contiguous()
                           or po.device != Q.device):
        raise ValueError("pos_offsets must be a dense int32 device tensor [B, Sq] on the device of Q")
    with torch.cuda.device(Q.device):
        if Q_out is None:
            s = stream if stream is not None else torch.cuda.current_stream()
            with torch.cuda.stream(s):
                Q_out = torch.empty((Sq, Q.shape[1], d), dtype=Q.dtype, device=Q.device).unsqueeze(0).transpose(1, 2) if ragged \
                    else torch.empty(Q.shape, dtype=Q.dtype, device=Q.device)
        st = [_strides(x) for x in (Q, K_new, V_new, Q_out, K, V)]
        symbol = _ROPE_SYMBOLS[paged, ragged] if po is None else _ROPE_POS_SYMBOLS[paged]
        rc = getattr(lib(), symbol)(
            Q.data_ptr(), K_new.data_ptr(), V_new.data_ptr(), Q_out.data_ptr(), K.data_ptr(), V.data_ptr(), t.data_ptr(),
            *(() if po is None else (po.data_ptr(),)), *((ptr(cu_seqlens_q),) if ragged else ()), ptr(kv_lens), *map(ptr, tables), ptr(k_descale), ptr(v_descale), B, Q.shape[1], Hkv,
            Sq, *geometry, d, rot_dim, max_pos, int(bool(interleaved)), _dtype_code(K_new.dtype), _dtype_code(K.dtype),
            *[ctypes.byref(x) for x in st], _stream_ptr(stream))
    _check(rc)
    return Q_out.transpose(1, 2).squeeze(0) if ragged else Q_out


def kv_cache_append(K_new, V_new, K_cache, V_cache, kv_lens=None, k_descale=None, v_descale=None, stream=None):
    """Write the new rows of every sequence into the K/V caches ``flash_attention_decode`` reads, in place.  Returns None.

    ``K_new``, ``V_new``: bf16 ``[B, Hkv, Sq, d]`` device tensors, d = 64 or 128, 1 <= Sq <= capacity (not capped at
    FA_DECODE_MAX_Q: the same call fills a cache after a prefill); strided views are accepted (last dimension contiguous), so the
    K and V slices of a fused projection pass without a copy.  ``K_cache``, ``V_cache``: ``[B, Hkv, capacity, d]``, bf16 (a bit
    copy) or ``torch.float8_e4m3fn`` with ``k_descale`` / ``v_descale`` (fp32 device tensors ``[Hkv]``, None = 1): the stored byte
    is the e4m3fn code of ``clamp(x.float() / descale[kvh], -448, 448)``, rounded to nearest even once; +-inf stores +-448, NaN a
    NaN code, and the sign of zero is kept.

    Positions: the rows are the LAST Sq rows of the sequence and ``kv_lens[b]`` (int32 device tensor ``[B]``, None = the capacity)
    already counts them: with ``L = min(kv_lens[b], capacity)`` row i goes to position ``L - Sq + i``, written if that is >= 0;
    ``kv_lens[b] <= 0`` writes nothing.  A decode step is ``kv_lens += Sq; kv_cache_append(...); flash_attention_decode(...,
    is_causal=True)`` on one tensor of lengths.  Lengths and descales are read by the kernel: the call never synchronises and a
    captured graph sees the values of the moment.  Asynchronous on ``stream`` (default: torch's current stream).  No CPU fallback."""
    _append_front("kv_cache_append", K_new, V_new, K_cache, V_cache, None, None, kv_lens, k_descale, v_descale, stream)


def kv_cache_append_paged(K_new, V_new, K_pool, V_pool, block_table, kv_lens=None, k_descale=None, v_descale=None, stream=None):
    """``kv_cache_append`` into PAGED caches: pools ``[P, Hkv, page, d]`` (bf16 or float8_e4m3fn; page a power of two >= 16; strided
    views accepted, so a ``[P, page, Hkv, d]`` pool is ``pool.transpose(1, 2)``) and ``block_table``, an int32 device tensor
    ``[B, max_pages]`` with a contiguous last dimension (a row slice of a wider table is fine).  Position p of sequence b is row
    ``p % page`` of page ``block_table[b, p // page]``; the capacity is ``max_pages * page``.

    Only the entries of pages that receive a row are read, by the kernel.  An entry outside [0, P) is NOT clamped (decode may
    clamp: it only reads): the rows that would go to that page are skipped and nothing else is touched.  Two sequences that write
    the same row of one page: the winner is unspecified.  Everything else as for ``kv_cache_append``.  Returns None."""
    _append_front("kv_cache_append_paged", K_new, V_new, K_pool, V_pool, block_table, None, kv_lens, k_descale, v_descale, stream)


def kv_cache_append_varlen(K_new, V_new, K_cache, V_cache, cu_seqlens_q, kv_lens=None, k_descale=None, v_descale=None, stream=None):
    """RAGGED ``kv_cache_append``: the new rows of a mixed batch, packed by token -- ``K_new``, ``V_new`` bf16 ``[T, Hkv, d]`` (strided
    views accepted, last dimension contiguous) with ``cu_seqlens_q`` (int32 device tensor ``[B + 1]``: the one
    ``flash_attention_extend_varlen`` takes) -- go into the caches ``[B, Hkv, capacity, d]``.  Per sequence, with ``sq_b`` its row
    count and ``L = min(kv_lens[b], capacity)``: row i goes to position ``L - sq_b + i`` when that is >= 0; ``L <= 0`` or
    ``sq_b == 0`` writes nothing; rows beyond ``cu[-1]`` are not read.  The bytes written for a sequence are those of
    ``kv_cache_append`` for that sequence alone; every other byte keeps its value.  T is not capped at the capacity.  A step of a
    mixed batch is ``kv_lens += q_lens; kv_cache_append_varlen(...); flash_attention_extend_varlen(..., is_causal=True)``, one
    graph.  Returns None.  No CPU fallback."""
    _append_front("kv_cache_append_varlen", K_new, V_new, K_cache, V_cache, None, cu_seqlens_q, kv_lens, k_descale, v_descale, stream)


def kv_cache_append_paged_varlen(K_new, V_new, K_pool, V_pool, block_table, cu_seqlens_q, kv_lens=None, k_descale=None, v_descale=None,
                                 stream=None):
    """``kv_cache_append_varlen`` into PAGED caches: the pools and the ``block_table`` ``[B, max_pages]`` of ``kv_cache_append_paged``,
    with that call's rules -- only the entries of pages that receive a row are read, an entry outside [0, P) is skipped and never
    clamped.  Returns None."""
    _append_front("kv_cache_append_paged_varlen", K_new, V_new, K_pool, V_pool, block_table, cu_seqlens_q, kv_lens, k_descale, v_descale,
                  stream)


def rope_table(max_pos, rot_dim, base=10000.0, device=None):
    """The cos / sin table the ``rope_cache_append*`` calls read: fp32 ``[max_pos, rot_dim]``, row p = ``cos(p * theta_j)`` for
    ``j < rot_dim / 2`` then ``sin(p * theta_j)``, ``theta_j = base ** (-2 j / rot_dim)`` -- computed in float64 and rounded once.
    Any other frequency rule (NTK, YaRN, ...) is a table of the caller's own in this layout."""
    import torch
    if rot_dim < 2 or rot_dim % 2 or max_pos < 1:
        raise ValueError("rope_table: max_pos >= 1 and an even rot_dim")
    theta = float(base) ** (-torch.arange(0, rot_dim, 2, dtype=torch.float64) / rot_dim)
    angle = torch.arange(max_pos, dtype=torch.float64)[:, None] * theta[None, :]
    return torch.cat([angle.cos(), angle.sin()], dim=1).to(torch.float32).to(device)


def rope_cache_append(Q, K_new, V_new, K_cache, V_cache, cos_sin, kv_lens=None, interleaved=False, k_descale=None, v_descale=None,
                      Q_out=None, stream=None, pos_offsets=None):
    """``kv_cache_append`` with the rotary embedding fused in: ONE launch rotates the new K rows at their cache positions and stores
    them into ``K_cache`` (bf16 or float8_e4m3fn), appends ``V_new`` exactly as ``kv_cache_append`` does, and rotates the step's query
    rows ``Q`` (bf16 ``[B, H, Sq, d]``, Hkv dividing H; strided views accepted) at the same positions.  Returns the rotated queries:
    ``Q_out`` (None allocates; ``Q_out=Q`` rotates in place).

    ``cos_sin``: fp32 device tensor ``[max_pos, rot_dim]`` (``rope_table``): row p is ``cos(p theta_j)``, ``j < rot_dim / 2``, then
    ``sin(p theta_j)``; rot_dim a multiple of 16 up to d (columns beyond it pass through), max_pos at least the capacity.
    ``interleaved``: False = NeoX pairs ``(j, j + rot_dim / 2)``, True = GPT-J pairs ``(2j, 2j + 1)``.

    Positions: K and V as in ``kv_cache_append``; Q row i is rotated at ``max(clamp(kv_lens[b], 1, capacity) - Sq + i, 0)``, the
    position ``flash_attention_decode`` / ``flash_attention_extend`` give it, and every Q row is written.  Values:
    ``y1 = fma(x1, c, -(x2 s))``, ``y2 = fma(x2, c, x1 s)`` in fp32, rounded once to bf16; K then goes through ``kv_cache_append``'s
    value rule, so the caches equal ``kv_cache_append`` of the bf16 rotation of K, byte for byte.  A decode step is ``kv_lens += Sq;
    Qr = rope_cache_append(...); flash_attention_decode(Qr, ...)``, one graph.  No CPU fallback.

    ``pos_offsets``: None, or an int32 device tensor ``[B, Sq]`` read by the kernel: row i (Q and K) is then rotated at
    ``max(first + clamp(pos_offsets[b, i], 0, Sq - 1), 0)``, ``first = clamp(kv_lens[b], 1, capacity) - Sq``, in place of
    ``first + i``; the row's SLOT, V and everything else are unchanged, and ``pos_offsets[b, i] = i`` is the call without it.  For a
    draft tree pass ``tree_depths(parents)``: a speculative step is ``kv_lens += Sq; Qr = rope_cache_append(..., pos_offsets=depths);
    flash_attention_tree(Qr, ...); (sampling); kv_cache_accept(..., *tree_path(parents, leaf)); kv_lens -= Sq - accept_lens``."""
    return _append_front("rope_cache_append", K_new, V_new, K_cache, V_cache, None, None, kv_lens, k_descale, v_descale, stream,
                         rope=(Q, Q_out, cos_sin, interleaved), pos_offsets=pos_offsets)


def rope_cache_append_paged(Q, K_new, V_new, K_pool, V_pool, block_table, cos_sin, kv_lens=None, interleaved=False, k_descale=None,
                            v_descale=None, Q_out=None, stream=None, pos_offsets=None):
    """``rope_cache_append`` into the PAGED caches of ``kv_cache_append_paged`` (max_pos at least ``max_pages * page``).  A table
    entry outside [0, P) skips the K and V rows of its page; their Q rows are still written.  ``pos_offsets`` as there."""
    return _append_front("rope_cache_append_paged", K_new, V_new, K_pool, V_pool, block_table, None, kv_lens, k_descale, v_descale, stream,
                         rope=(Q, Q_out, cos_sin, interleaved), pos_offsets=pos_offsets)


def rope_cache_append_varlen(Q, K_new, V_new, K_cache, V_cache, cu_seqlens_q, cos_sin, kv_lens=None, interleaved=False, k_descale=None,
                             v_descale=None, Q_out=None, stream=None):
    """RAGGED ``rope_cache_append``: ``Q`` ``[T, H, d]`` and ``K_new``, ``V_new`` ``[T, Hkv, d]`` packed by token with ``cu_seqlens_q``,
    as in ``kv_cache_append_varlen``; returns the rotated queries ``[T, H, d]``.  Every token a sequence owns is written; tokens
    nobody owns are neither read nor written (a ``Q_out`` allocated here holds unspecified values there).  A step of a mixed batch is
    ``kv_lens += q_lens; Qr = rope_cache_append_varlen(...); flash_attention_extend_varlen(Qr, ...)``."""
    return _append_front("rope_cache_append_varlen", K_new, V_new, K_cache, V_cache, None, cu_seqlens_q, kv_lens, k_descale, v_descale, stream,
                         rope=(Q, Q_out, cos_sin, interleaved))


def rope_cache_append_paged_varlen(Q, K_new, V_new, K_pool, V_pool, block_table, cu_seqlens_q, cos_sin, kv_lens=None, interleaved=False,
                                   k_descale=None, v_descale=None, Q_out=None, stream=None):
    """``rope_cache_append_varlen`` into PAGED caches: the pools and the table of ``kv_cache_append_paged``."""
    return _append_front("rope_cache_append_paged_varlen", K_new, V_new, K_pool, V_pool, block_table, cu_seqlens_q, kv_lens, k_descale, v_descale, stream,
                         rope=(Q, Q_out, cos_sin, interleaved))


def _library_accepts(t):
    """What the C ABI asks of a [B, H, S, d] view (csrc/FlashAttention.hip: strides_ok, aligned16): last dimension contiguous, rows
    that do not overlap, every stride a multiple of 16 bytes, a 16-byte aligned base."""
    esz = t.element_size()
    sB, sH, sS, sD = t.stride()
    return (sD == 1 and sS >= t.shape[3] and sB >= 0 and sH >= 0 and all((s * esz) % 16 == 0 for s in (sB, sH, sS))
            and t.data_ptr() % 16 == 0)


def _attention_function():
    import torch

    class _Attention(torch.autograd.Function):
        @staticmethod
        def forward(ctx, Q, K, V, is_causal, scale, out_dtype):
            O, lse = flash_attention(Q, K, V, scale=scale, is_causal=is_causal, out_dtype=out_dtype, return_lse=True)
            ctx.save_for_backward(Q, K, V, O, lse)
            ctx.is_causal, ctx.scale = is_causal, scale
            return O

        @staticmethod
        def backward(ctx, dO):
            Q, K, V, O, lse = ctx.saved_tensors
            dO = dO.to(O.dtype)
            # autograd hands back whatever view the loss produced (expanded: strideS = 0; narrowed: any row stride): copy exactly when
            # the library would refuse it, pass every other view (a model-layout dO) through
            if not _library_accepts(dO):
                dO = dO.contiguous()
            dQ, dK, dV = flash_attention_backward(Q, K, V, O, dO, lse, scale=ctx.scale, is_causal=ctx.is_causal)
            return dQ.to(Q.dtype), dK.to(K.dtype), dV.to(V.dtype), None, None, None

    return _Attention


_AttentionFn = None


def attention(Q, K, V, is_causal=False, scale=None, out_dtype=None):
    """Differentiable O = softmax(scale * Q K^T [+ causal mask]) V: the forward is ``flash_attention(..., return_lse=True)``, the
    backward ``flash_attention_backward`` (bf16 inputs, d = 64 / 128 for the backward; gradients in the inputs' type).  K and V
    may hold fewer heads than Q (grouped-query attention, see ``flash_attention``); their gradients are shaped like them."""
    global _AttentionFn
    if _AttentionFn is None:
        _AttentionFn = _attention_function()
    if scale is None:
        scale = 1.0 / float(Q.shape[-1]) ** 0.5
    return _AttentionFn.apply(Q, K, V, bool(is_causal), float(scale), out_dtype)
