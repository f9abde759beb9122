"""CPU tests of the speculative step's write side -- flash_attention_rope_append_pos, _paged_pos, flash_attention_kv_accept, _paged -- at
the C ABI and in the binding, and of the reference the GPU tests compare with (tests/spec_step_check.py):

* the four symbols exist with the declared parameter lists and argtypes, each list its twin's plus or minus what the header names;
* the _pos ladder returns its rope_append twin's code on every rung of the twin's ladder, and refuses posOffsets at its two places;
* the accept ladder beside the append's (a cache the append accepts, accept accepts), and its own rungs; the binding's refusals
  (aligned host pointers: no GPU is touched, and no case is valid as a whole);
* tree_path against an ancestor walk;
* the reference: identity offsets are rope_check.rope_append; accept(rope_append_pos(depths), tree_path(leaf)) is the linear rotary
  append of the accepted tokens, byte for byte, bf16 and fp8, contiguous and paged; nine wrong kernels, emulated, are each refused on
  a named tensor and row."""
import ctypes
import re

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import rope_check as rc  # noqa: E402
import spec_step_call as call  # noqa: E402
import spec_step_check as sp  # noqa: E402
from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SHAPE, BAD_STRIDE, BF16, F16, F32, FA_ERR, FP8, MISALIGNED, NULL_POINTER,  # noqa: E402
                      MetaTensor as T, aligned_host_pointer, declared_parameters, host_call)
from kv_append_check import descales, sentinel  # noqa: E402
from kv_cache_check import gather  # noqa: E402
from rope_check import rows, table_of  # noqa: E402

BAD_FLAGS = FA_ERR["BAD_FLAGS"]
B, HKV, CAP = 2, 2, 384


# ---- 1. the symbols ----
def test_the_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    sp_, vp, i = ctypes.POINTER(fa.FaStrides), ctypes.c_void_p, ctypes.c_int
    kinds = {"batchSize": i, "numHeads": i, "numHeadsKV": i, "seqLenNew": i, "seqLenDraft": i, "seqLenK": i, "numPages": i, "pageSize": i,
             "maxPagesPerSeq": i, "tableStride": ctypes.c_int64, "dHead": i, "rotDim": i, "maxPos": i, "interleaved": i, "dtype": i,
             "kv_dtype": i, "sQ": sp_, "sKnew": sp_, "sVnew": sp_, "sQout": sp_, "sK": sp_, "sV": sp_}
    for paged in (False, True):
        for name in (call.ROPE_POS[paged], call.ACCEPT[paged]):
            assert name in fa.EXPORTS and getattr(L, name) is not None
            assert list(getattr(L, name).argtypes) == [kinds.get(p, vp) for p in declared_parameters(name)], name
            assert getattr(L, name).restype is i
        # the rope twin's list with posOffsets directly after cosSin
        want = declared_parameters(call.ROPE_TWIN[paged])
        want.insert(want.index("cosSin") + 1, "posOffsets")
        assert declared_parameters(call.ROPE_POS[paged]) == want
        # the append's list without the new rows, their strides, the descales and dtype; seqLenDraft for seqLenNew; the two arrays
        # after kvLens (paged: after the table)
        want = [p for p in declared_parameters(call.APPEND[paged]) if p not in ("Knew", "Vnew", "sKnew", "sVnew", "kDescale", "vDescale", "dtype")]
        want[want.index("seqLenNew")] = "seqLenDraft"
        at = want.index("blockTable" if paged else "kvLens") + 1
        want[at:at] = ["acceptIdx", "acceptLens"]
        assert declared_parameters(call.ACCEPT[paged]) == want
    assert fa.FA_TREE_MAX_Q == 64


# ---- 2. the _pos ladder ----
def rope_calls(kv):
    """(pos call, twin call, p) per form on one aligned host pointer: valid as a whole, so every use overrides something"""
    host = aligned_host_pointer()
    p = host[1]
    okc = dict(B=2, H=8, Hkv=2, Sq=3, Sk=1024, d=128, rot=64, maxpos=1024, il=0, dtype=BF16, kv=kv, pos=p)
    okp = dict(B=2, H=8, Hkv=2, Sq=3, P=64, page=64, maxp=16, ts=16, d=128, rot=64, maxpos=1024, il=0, dtype=BF16, kv=kv, pos=p)
    return [(paged, host_call(call.ROPE_POS[paged], okp if paged else okc, host)[0]) for paged in (False, True)], p


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_the_pos_ladder_is_the_twins_code_for_code(kv):
    forms, p = rope_calls(kv)
    esz = 2 if kv == BF16 else 1
    low = fa.FaStrides(1 << 20, 1 << 16, 56)
    for paged, c in forms:
        twin = call.ROPE_TWIN[paged]
        rungs = [dict(Kn=None), dict(V=None, K=p + 8), dict(Q=None), dict(Qo=None), dict(cs=None), dict(cs=None, Kn=p + 8),
                 dict(Vn=p + 8), dict(K=p + 8, Sq=0), dict(Q=p + 8), dict(Qo=p + 4), dict(cs=p + 8, Sq=0), dict(lens=p + 2, d=96),
                 dict(lens=p + 4, d=96), dict(kd=p + 2, d=96), dict(vd=p + 2, d=96), dict(Sq=0), dict(Sq=-1), dict(B=0), dict(Hkv=0), dict(d=0),
                 dict(B=1 << 16, Hkv=1 << 15, H=1 << 15), dict(Sq=1025, d=96), dict(H=0), dict(H=7), dict(H=7, dtype=F32), dict(H=7, d=96),
                 dict(dtype=F32, d=96), dict(dtype=FP8, d=96), dict(kv=F16, d=96), dict(kv=-1), dict(kd=p, d=96), dict(kd=p, vd=p + 4, d=96),
                 dict(d=96), dict(d=32), dict(d=256), dict(rot=0), dict(rot=24), dict(rot=144), dict(rot=24, d=96), dict(rot=24, kv=F16),
                 dict(d=64, rot=128), dict(maxpos=1023), dict(maxpos=0), dict(maxpos=1023, il=2), dict(il=2), dict(il=-1), dict(il=1, d=96)]
        for at in range(6):                                   # sQ, sKnew, sVnew, sQout, sK, sV
            st = [None] * 6
            st[at] = ctypes.byref(low)
            rungs += [dict(strides=st, d=64, rot=64), dict(strides=st, il=2)]
        if paged:
            rungs += [dict(table=None), dict(table=p + 2, d=96), dict(Q=p + 8, page=24), dict(P=0), dict(maxp=0), dict(page=8), dict(page=24), dict(ts=15),
                      dict(page=(1 << 31) // (128 * esz), maxp=1, ts=1, maxpos=1 << 25),
                      dict(strides=[ctypes.byref(low)] + [None] * 5, page=(1 << 31) // 128, maxp=1, ts=1, maxpos=1 << 25)]
        else:
            rungs += [dict(Sk=0), dict(Sk=-128), dict(Sk=(1 << 24) + 1, maxpos=1 << 25), dict(Sk=(1 << 31) // (128 * esz) - 192, maxpos=1 << 25),
                      dict(strides=[ctypes.byref(low)] + [None] * 5, Sk=(1 << 31) // 128 - 192, maxpos=1 << 25)]
        seen = set()
        for kw in rungs:
            want = c(symbol=twin, **kw)
            assert want != 0 and c(**kw) == want, (paged, kw, want)
            seen.add(want)
        assert seen == {NULL_POINTER, MISALIGNED, BAD_SHAPE, BAD_DTYPE, BAD_DHEAD, BAD_FLAGS, BAD_STRIDE}
        # posOffsets: NULL with the other pointers, before any alignment check; 4 bytes with the other 4-byte arrays -- after the
        # 16-byte checks, before the paging geometry and the shape
        assert c(pos=None) == NULL_POINTER and c(pos=None, Kn=p + 8) == NULL_POINTER and c(pos=None, lens=p + 2) == NULL_POINTER
        for off in (1, 2, 3):
            assert c(pos=p + off) == MISALIGNED and c(pos=p + off, Sq=0) == MISALIGNED and c(pos=p + off, d=96) == MISALIGNED, off
            if paged:
                assert c(pos=p + off, page=24) == MISALIGNED
        for off in (4, 8, 12):                                # 4 bytes is all it needs: the call passes on to the next rung
            assert c(pos=p + off, Sq=0) == BAD_SHAPE and c(pos=p + off, d=96) == BAD_DHEAD, off
        assert c(pos=p + 2, Q=p + 8) == MISALIGNED and c(pos=p + 4, Q=None) == NULL_POINTER


# ---- 3. the accept ladder ----
def accept_calls():
    host = aligned_host_pointer()
    p = host[1]
    okc = dict(B=2, Hkv=2, draft=5, Sq=5, Sk=1024, d=128, dtype=BF16, idx=p, nacc=p)
    okp = dict(B=2, Hkv=2, draft=5, Sq=5, P=64, page=64, maxp=16, ts=16, d=128, dtype=BF16, idx=p, nacc=p)
    return [(paged, host_call(call.ACCEPT[paged], okp if paged else okc, host)[0]) for paged in (False, True)], p


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_the_accept_ladder_beside_the_appends(kv):
    forms, p = accept_calls()
    esz = 2 if kv == BF16 else 1
    low, odd = fa.FaStrides(1 << 20, 1 << 16, 56), fa.FaStrides(-7, 1 << 16, 128)
    for paged, c0 in forms:
        c = lambda **kw: c0(**dict(dict(kv=kv), **kw))        # noqa: E731
        append = call.APPEND[paged]
        # what both calls take, the append refuses and accept refuses alike: Sq and draft are the two names of one row count
        both = [dict(K=None), dict(V=None, K=p + 8), dict(K=p + 8), dict(V=p + 8, Sq=0, draft=0), dict(lens=p + 2, d=96), dict(lens=p + 4, d=96),
                dict(Sq=0, draft=0), dict(Sq=-1, draft=-1), dict(B=0), dict(Hkv=0), dict(d=0), dict(B=1 << 16, Hkv=1 << 15), dict(Sq=0, draft=0, kv=F16),
                dict(kv=F16, d=96), dict(kv=F32), dict(kv=-1), dict(d=96), dict(d=32), dict(d=256)]
        for s in (low, odd):
            both += [dict(strides=[None, None, ctypes.byref(s), None], d=64), dict(strides=[None, None, None, ctypes.byref(s)], d=64),
                     dict(strides=[None, None, ctypes.byref(s), None], d=96)]
        if paged:
            both += [dict(table=None), dict(table=p + 2, d=96), dict(K=p + 8, page=24), dict(P=0), dict(maxp=0), dict(page=8), dict(page=24), dict(ts=15),
                     dict(page=16, maxp=(1 << 20) + 1, ts=1 << 21), dict(page=(1 << 31) // (128 * esz), maxp=1, ts=1),
                     dict(page=4, maxp=1, ts=1, Sq=5, draft=5)]
        else:
            both += [dict(Sk=0), dict(Sk=-128), dict(Sk=(1 << 24) + 1), dict(Sk=(1 << 31) // (128 * esz) - 192), dict(Sk=4)]
        seen = set()
        for kw in both:
            akw = {k: v for k, v in kw.items() if k != "strides"}
            if "strides" in kw:
                akw["strides"] = kw["strides"][2:]             # (sK, sV of the append's sKnew, sVnew, sK, sV)
            want = c(symbol=append, **kw)
            assert want != 0 and c(**akw) == want, (paged, kw, want)
            seen.add(want)
        assert seen == {NULL_POINTER, MISALIGNED, BAD_SHAPE, BAD_DTYPE, BAD_DHEAD, BAD_STRIDE}
        # its own: the two arrays with the pointers and with the 4-byte arrays; the draft's cap with the shape
        for name in ("idx", "nacc"):
            assert c(**{name: None}) == NULL_POINTER and c(**{name: None}, K=p + 8) == NULL_POINTER, name
            for off in (1, 2, 3):
                assert c(**{name: p + off}) == MISALIGNED and c(**{name: p + off}, draft=0) == MISALIGNED, (name, off)
                if paged:
                    assert c(**{name: p + off}, page=24) == MISALIGNED
            assert c(**{name: p + 4}, d=96) == BAD_DHEAD and c(**{name: p + 2}, K=p + 8) == MISALIGNED
        for n in (fa.FA_TREE_MAX_Q + 1, 100, 1024, 1025):
            assert c(draft=n) == BAD_SHAPE and c(draft=n, kv=F16) == BAD_SHAPE and c(draft=n, d=96) == BAD_SHAPE, n
        for n in (1, 16, 17, fa.FA_TREE_MAX_Q):
            assert c(draft=n, d=96) == BAD_DHEAD, n            # every draft size up to the cap passes on
        small = dict(page=16, maxp=2, ts=2) if paged else dict(Sk=32)
        assert c(draft=33, **small) == BAD_SHAPE and c(draft=32, d=96, **small) == BAD_DHEAD      # above the capacity


def test_binding_refusals():
    f8, bf, i32 = torch.float8_e4m3fn, torch.bfloat16, torch.int32
    k, pool = torch.zeros(2, 2, 32, 64, dtype=bf), torch.zeros(6, 2, 16, 64, dtype=bf)
    table = torch.zeros(2, 2, dtype=i32)
    idx, n = torch.zeros(2, 5, dtype=i32), torch.zeros(2, dtype=i32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.kv_cache_accept(k, k, idx, n)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.kv_cache_accept_paged(T(pool), T(pool), T(table), idx, T(n))

    def both(K=k, Kp=pool, table_=table, idx_=idx, n_=n, V=None, **kw):
        yield lambda: fa.kv_cache_accept(T(K), T(K if V is None else V), T(idx_), T(n_), **kw)
        yield lambda: fa.kv_cache_accept_paged(T(Kp), T(Kp if V is None else V), T(table_), T(idx_), T(n_), **kw)

    for c in both(K=k[0], Kp=pool[0]):
        with pytest.raises(ValueError, match="of one dtype"):
            c()
    for c in both(V=torch.zeros(2, 2, 32, 64, dtype=f8)):
        with pytest.raises(ValueError, match="of one dtype"):
            c()
    for c in both(K=k.float(), Kp=pool.half()):
        with pytest.raises(TypeError, match="bfloat16 or float8_e4m3fn"):
            c()
    for bad in (idx.long(), idx[0], torch.zeros(2, 10, dtype=i32)[:, ::2]):
        for c in both(idx_=bad):
            with pytest.raises(ValueError, match="accept_idx"):
                c()
    for bad in (n.long(), torch.zeros(3, dtype=i32), torch.zeros(2, 1, dtype=i32), torch.zeros(4, dtype=i32)[::2]):
        for c in both(n_=bad):
            with pytest.raises(ValueError, match="accept_lens"):
                c()
    with pytest.raises(ValueError, match="the batch of accept_idx"):
        fa.kv_cache_accept(T(k), T(k), T(torch.zeros(3, 5, dtype=i32)), T(torch.zeros(3, dtype=i32)))
    with pytest.raises(ValueError, match="block_table"):
        fa.kv_cache_accept_paged(T(pool), T(pool), T(table.long()), T(idx), T(n))
    for Sq in (0, 33, 65):                                     # none, above the capacity (32 both ways), above FA_TREE_MAX_Q
        for c in both(idx_=torch.zeros(2, Sq, dtype=i32)):
            with pytest.raises(ValueError, match="draft nodes"):
                c()
    for c in both(kv_lens=T(torch.zeros(3, dtype=i32))):
        with pytest.raises(ValueError, match="kv_lens"):
            c()
    with pytest.raises(ValueError, match="accept_idx"):
        fa.kv_cache_accept(T(k), T(k), T(idx, device="cuda:1"), T(n))
    # pos_offsets of the rope fronts: a dense int32 [B, Sq] device tensor on Q's device
    q, new, cs = torch.zeros(2, 4, 3, 64, dtype=bf), torch.zeros(2, 2, 3, 64, dtype=bf), torch.zeros(32, 32)
    bads = [T(t) for t in (torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 4, dtype=i32), torch.zeros(3, dtype=i32),
                           torch.zeros(2, 6, dtype=i32)[:, ::2])] + [T(torch.zeros(2, 3, dtype=i32), device="cuda:1"), torch.zeros(2, 3, dtype=i32)]
    for po in bads:
        with pytest.raises(ValueError, match="pos_offsets"):
            fa.rope_cache_append(T(q), T(new), T(new), T(k), T(k), T(cs), pos_offsets=po)
        with pytest.raises(ValueError, match="pos_offsets"):
            fa.rope_cache_append_paged(T(q), T(new), T(new), T(pool), T(pool), T(table), T(cs), pos_offsets=po)


# ---- 4. tree_path ----
def test_tree_path_is_the_ancestor_walk():
    for Sq in (1, 2, 7, 33, 64):
        trees = [sp.binary(Sq), sp.star(Sq), sp.chain(Sq)] + [sp.random_tree(Sq, 10 * Sq + s) for s in range(3)]
        for leaves in ([0] * len(trees), [Sq - 1] * len(trees), [(3 * k + Sq // 2) % Sq for k in range(len(trees))]):
            idx, n = fa.tree_path(torch.tensor(trees), torch.tensor(leaves))
            assert idx.dtype == torch.int32 and n.dtype == torch.int32 and idx.shape == (len(trees), Sq) and n.shape == (len(trees),)
            dep = fa.tree_depths(trees)
            for b, (parents, leaf) in enumerate(zip(trees, leaves)):
                want, count = sp.tree_path(parents, leaf)
                assert idx[b].tolist() == want and int(n[b]) == count == int(dep[b, leaf]) + 1, (Sq, b, leaf)
                assert want[0] == 0 or parents[want[0]] == -1
                assert all(want[t] < want[t + 1] for t in range(count - 1))            # strictly increasing: j_t >= t
    # leaves out of range are clamped into the tree; lists are taken; the checks of the parent array are tree_mask_from_parents'
    idx, n = fa.tree_path([sp.binary(7)] * 2, torch.tensor([-4, 99]))
    assert idx.tolist() == [[0] + [6] * 6, [0, 2, 6, 6, 6, 6, 6]] and n.tolist() == [1, 3]
    for bad in ([[0, 0]], [[-1, 1]], [[-1, -2]], [[-1.0, 0.0]]):
        with pytest.raises(ValueError):
            fa.tree_path(bad, torch.tensor([0]))
    for bad in (torch.tensor([0, 0]), torch.tensor([[0]]), torch.tensor([0.0])):
        with pytest.raises(ValueError, match="leaf"):
            fa.tree_path([sp.binary(3)], bad)


# ---- 5. the reference ----
def scene(Sq, d, fp8, page, lens, seed, G=2):
    """(Q, Kn, Vn, Kc, Vc, table, kd, vd, bt) on the CPU: sentinel caches of capacity CAP, contiguous or (page) paged"""
    Q, Kn, Vn = rows((B, HKV * G, Sq, d), seed), rows((B, HKV, Sq, d), seed + 1), rows((B, HKV, Sq, d), seed + 2)
    kd, vd = descales(seed + 3, fp8, HKV)
    if page:
        P, bt = table_of(B, CAP // page, 3, seed + 4)
        Kc, Vc = sentinel((P, HKV, page, d), fp8), sentinel((P, HKV, page, d), fp8)
    else:
        bt, Kc, Vc = None, sentinel((B, HKV, CAP, d), fp8), sentinel((B, HKV, CAP, d), fp8)
    return Q, Kn, Vn, Kc, Vc, fa.rope_table(CAP, d // 2), kd, vd, bt


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [None, 16, 128])
def test_identity_offsets_are_the_twin(page, fp8):
    for Sq, lens in ((1, [0, 17]), (7, [3, 384]), (31, [130, 31]), (64, [400, 65])):
        Q, Kn, Vn, Kc, Vc, table, kd, vd, bt = scene(Sq, 64, fp8, page, lens, 40 + Sq)
        for L in (lens, None):
            got = sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, L, [list(range(Sq))] * B, True, kd, vd, bt)
            want = rc.rope_append(Q, Kn, Vn, Kc, Vc, table, L, True, kd, vd, bt)[:3]
            assert all(torch.equal(rc.bits(g), rc.bits(w)) for g, w in zip(got, want)), (Sq, L)   # difference 0
    # the clamp: offsets out of range are the call on the clamped values
    Q, Kn, Vn, Kc, Vc, table, kd, vd, bt = scene(7, 64, fp8, page, [50, 5], 60)
    a = sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, [50, 5], [[-5, 16, 2 ** 31 - 1, 3, 0, 6, 7]] * B, False, kd, vd, bt)
    b = sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, [50, 5], [[0, 6, 6, 3, 0, 6, 6]] * B, False, kd, vd, bt)
    assert all(torch.equal(rc.bits(x), rc.bits(y)) for x, y in zip(a, b))
    assert sp.pos_positions(5, 7, CAP, [0, 6, 1, 2, 2, 3, 9]) == [0, 4, 0, 0, 0, 1, 4]           # first = -2: max(first + off, 0)


def below(cache, bt, b, n):
    """the rows [0, n) of sequence b: [Hkv, n, d]"""
    return (cache if bt is None else gather(cache, bt))[b, :, :n]


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [None, 16, 128])
@pytest.mark.parametrize("d", [64, 128])
def test_accepting_a_depth_rotated_tree_is_the_linear_append(d, page, fp8):
    """THE KEY IDENTITY: accept(rope_append_pos(depths), tree_path(leaf)) equals, on the rows [0, base + n), rope_check.rope_append of
    the accepted tokens appended linearly, byte for byte"""
    for Sq, family, starts, il in ((7, "binary", (100, 250), False), (15, "star", (0, 369), True), (33, "random", (120, 15), False),
                                   (64, "random", (130, 320), True), (5, "binary", (-2, 127), False)):
        trees = [{"binary": sp.binary, "star": sp.star}[family](Sq) if family != "random" else sp.random_tree(Sq, 70 + Sq + b) for b in range(B)]
        lens = [s + Sq for s in starts]                      # (a start below zero: more draft nodes than the length counts)
        Q, Kn, Vn, Kc, Vc, table, kd, vd, bt = scene(Sq, d, fp8, page, lens, 80 + Sq)
        leaves = [Sq - 1, Sq // 2]
        idx, n = fa.tree_path(torch.tensor(trees), torch.tensor(leaves))
        _, K1, V1 = sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, lens, fa.tree_depths(trees).tolist(), il, kd, vd, bt)
        K2, V2 = sp.accept(K1, V1, lens, idx.tolist(), n.tolist(), Sq, bt)
        for b in range(B):
            path, count = idx[b, :int(n[b])].tolist(), int(n[b])
            base = min(lens[b], CAP) - Sq
            if base < 0:                                     # the draft's leading nodes were never written: nothing to compare with
                continue
            one = [base + count if x == b else 0 for x in range(B)]
            _, Kl, Vl, _ = rc.rope_append(Q[:, :, path], Kn[:, :, path], Vn[:, :, path], Kc, Vc, table, one, il, kd, vd, bt)
            for name, got, want in (("K", K2, Kl), ("V", V2, Vl)):
                g, w = below(got, bt, b, base + count), below(want, bt, b, base + count)
                assert torch.equal(g, w), (name, Sq, family, b)
            # ... and the draft's rows were all there before: the prefix is untouched, the rest of the cache too
            assert torch.equal(below(K2, bt, b, base), below(Kc, bt, b, base))
            assert torch.equal((K2 if bt is None else gather(K2, bt))[b, :, base + Sq:], (Kc if bt is None else gather(Kc, bt))[b, :, base + Sq:])


def first_bad(names, got, want):
    """(tensor name, (b, head, row, col)) of the first element that differs, tensors in the order given; None if none does"""
    for name, g, w in zip(names, got, want):
        text = sp.first_difference(name, g, w)
        if text:
            m = re.match(r"(\w+)\[(\d+), (\d+), (\d+), (\d+)\]", text)
            return m.group(1), tuple(int(x) for x in m.groups()[1:])
    return None


@pytest.mark.parametrize("fp8", [False, True])
def test_wrong_kernels_are_refused_on_a_named_tensor_and_row(fp8):
    Sq, d, lens = 7, 64, [107, 257]
    base = [L - Sq for L in lens]
    Q, Kn, Vn, Kc, Vc, table, kd, vd, _ = scene(Sq, d, fp8, None, lens, 90)
    offs = [sp.depths(sp.binary(Sq)), sp.depths(sp.star(Sq))]           # [0, 1, 1, 2, 2, 2, 2] and [0, 1, 1, 1, 1, 1, 1]
    right = sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, lens, offs, False, kd, vd)
    names = ("Qout", "Kcache", "Vcache")
    assert first_bad(names, right, right) is None
    # row = the Q row, or the cache position
    expect = {"offsets by cache position": ("Qout", 0, 0),              # first >= Sq: every row takes offs[b][Sq - 1] = 2, node 0 too
              "offsets of batch 0": ("Qout", 1, 3),                     # sequence 1 with the binary tree's depths: node 3
              "offset moves the slot": ("Kcache", 0, base[0] + 1),      # slot 1 holds node 2
              "Q at base + i": ("Qout", 0, 2)}                          # node 2 at depth 1 rotated at base + 2
    assert set(expect) == set(sp.WRONG_ROPE)
    for wrong, (tensor, b, row) in expect.items():
        got = sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, lens, offs, False, kd, vd, wrong=wrong)
        bad = first_bad(names, got, right)
        assert bad is not None and (bad[0], bad[1][0], bad[1][2]) == (tensor, b, row), (wrong, bad)
    assert torch.equal(sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, lens, offs, False, kd, vd, wrong="Q at base + i")[1], right[1])
    # accept: the chain 1, 2, 3, ... on sequence 0 (five moves), a binary tree's path on sequence 1 (three nodes)
    K1, V1 = right[1], right[2]
    idx = [[1, 2, 3, 4, 5, 6, 6], sp.tree_path(sp.binary(Sq), Sq - 1)[0]]
    nacc = [5, 3]
    good = sp.accept(K1, V1, lens, idx, nacc, Sq)
    for t in range(5):                                                   # the chain: row t is the draft's row t + 1
        assert torch.equal(good[0][0, :, base[0] + t], K1[0, :, base[0] + t + 1]) and torch.equal(good[1][0, :, base[0] + t], V1[0, :, base[0] + t + 1])
    expect = {"descending t": ("Kcache", 0, base[0]),                    # row 0 ends as the draft's row 5
              "parallel moves": ("Kcache", 0, base[0]),                  # move 0 reads row 1 after move 1 has written it
              "destination j_t": ("Kcache", 0, base[0]),                 # nothing moves at all
              "lens of the other sequence": ("Kcache", 0, base[0] + 3),  # three moves where five were due
              "V not moved": ("Vcache", 0, base[0])}
    assert set(expect) == set(sp.WRONG_ACCEPT)
    for wrong, (tensor, b, row) in expect.items():
        got = sp.accept(K1, V1, lens, idx, nacc, Sq, wrong=wrong)
        bad = first_bad(names[1:], got, good)
        assert bad is not None and (bad[0], bad[1][0], bad[1][2]) == (tensor, b, row), (wrong, bad)


def test_the_accept_reference_clamps_and_skips():
    Sq, d = 5, 64
    g = torch.Generator().manual_seed(7)
    Kc = torch.randint(-30000, 30000, (B, HKV, 32, d), generator=g, dtype=torch.int16)
    Vc = torch.randint(-30000, 30000, (B, HKV, 32, d), generator=g, dtype=torch.int16)
    # identity: no byte changes; n <= 0: nothing; n above Sq and indices out of range: the clamped call
    for idx, n in (([[0, 1, 2, 3, 4]] * B, [5, 5]), ([[4, 4, 4, 4, 4]] * B, [0, -3])):
        K2, V2 = sp.accept(Kc, Vc, [20, 32], idx, n, Sq)
        assert torch.equal(K2, Kc) and torch.equal(V2, Vc)
    a = sp.accept(Kc, Vc, [20, 32], [[-7, 2, 99, 4, 2 ** 31 - 1]] * B, [12, 5], Sq)
    b = sp.accept(Kc, Vc, [20, 32], [[0, 2, 4, 4, 4]] * B, [5, 5], Sq)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], Kc)
    # a length of zero: nothing; a draft that outnumbers the length: the moves with a negative position are skipped
    K2, _ = sp.accept(Kc, Vc, [0, 3], [[1, 2, 3, 4, 4]] * B, [4, 4], Sq)
    assert torch.equal(K2[0], Kc[0])
    want = Kc[1].clone()                                     # base = -2: moves 0, 1 have negative destinations; 2: row 0 := row 1; 3: row 1 := row 2
    want[:, 0], want[:, 1] = Kc[1][:, 1], Kc[1][:, 2]
    assert torch.equal(K2[1], want)
    # a pool: entries out of range skip the move on either side
    pool = torch.randint(-30000, 30000, (6, HKV, 16, d), generator=g, dtype=torch.int16)
    bt = torch.tensor([[4, 1], [0, 9]], dtype=torch.int32)
    K2, V2 = sp.accept(pool, pool, [20, 20], [[2, 3, 4, 4, 4]] * B, [3, 3], Sq, bt)     # base = 15: node 0 in page 0 of the sequence, the rest in page 1
    want = pool.clone()
    want[4, :, 15], want[1, :, 0], want[1, :, 1] = pool[1, :, 1], pool[1, :, 2], pool[1, :, 3]
    assert torch.equal(K2, want) and torch.equal(V2, want)   # (sequence 1: every source lies in the page of entry 9 -- skipped)
