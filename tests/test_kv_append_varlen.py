"""GPU tests of kv_cache_append_varlen and kv_cache_append_paged_varlen (flash_attention_kv_append_varlen, _paged_varlen): the ragged
cache append -- new rows packed by token, every sequence its own row count.

Everything here is a comparison of BITS.  The yardstick is the uniform append, one call per sequence (batch of one, seqLenNew = sq_b)
on a poisoned cache: the ragged call on the same poisoned cache must leave the same bytes, which pins every byte it must write and
every byte it must not.  One fp8 case is also held against tests/kv_append_check.py, the contract written in torch on the CPU.  The
caches are integer tensors (uint8: e4m3fn bytes, int16: bf16 patterns), as in tests/test_kv_append.py."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import kv_append_check as kc  # noqa: E402
from kv_append_check import SENT, as_cache, new_rows, same  # noqa: E402
from kv_cache_check import DEV, cu_of, i32 as t32  # noqa: E402

pytestmark = pytest.mark.gpu
bf, i16, u8, i32 = torch.bfloat16, torch.int16, torch.uint8, torch.int32
HKV = 2
PAD = 9                               # tokens beyond cu[-1]: not read


def sentinel(shape, fp8):
    return kc.sentinel(shape, fp8, DEV)


def descales(seed, fp8):
    kd, vd = kc.descales(seed, fp8)
    return dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV)) if fp8 else {}


def both_ways(sq, lens, cap, d, fp8, page, seed, table=None, strided=False):
    """(ragged K, ragged V, per-sequence K, per-sequence V): the caches after the ragged append and after the uniform append called
    once per sequence, both from the sentinel.  page None: contiguous [B, Hkv, cap, d]; else pools behind `table` (default: a shuffle)"""
    B, T = len(sq), sum(sq) + PAD
    cu = cu_of(sq)
    Kn, Vn = new_rows((T, HKV, d), seed).to(DEV), new_rows((T, HKV, d), seed + 1).to(DEV)
    if strided:      # the K and V slices of a fused [T, (H + 2 Hkv) d] projection
        fused = torch.zeros((T, (4 + 2 * HKV) * d), dtype=bf, device=DEV)
        fused[:, 4 * d:(4 + HKV) * d], fused[:, (4 + HKV) * d:] = Kn.reshape(T, -1), Vn.reshape(T, -1)
        Kn, Vn = fused[:, 4 * d:(4 + HKV) * d].view(T, HKV, d), fused[:, (4 + HKV) * d:].view(T, HKV, d)
        assert not Kn.is_contiguous()
    ds = descales(seed + 2, fp8)
    if page is None:
        shape = (B, HKV, cap, d)
    else:
        n = cap // page
        shape = (B * n + 4, HKV, page, d)
        if table is None:
            table = torch.randperm(shape[0], generator=torch.Generator().manual_seed(seed + 3))[:B * n].reshape(B, n).to(i32)
        table = table.to(DEV)
    Kr, Vr, Ku, Vu = (sentinel(shape, fp8) for _ in range(4))
    if page is None:
        fa.kv_cache_append_varlen(Kn, Vn, as_cache(Kr), as_cache(Vr), t32(cu), t32(lens), **ds)
    else:
        fa.kv_cache_append_paged_varlen(Kn, Vn, as_cache(Kr), as_cache(Vr), table, t32(cu), t32(lens), **ds)
    for b, s in enumerate(sq):
        if s == 0:
            continue
        keep = min(s, cap)         # (the uniform call takes 1 .. capacity rows; of more, the last `cap` are the ones that can land)
        kn = Kn[cu[b + 1] - keep:cu[b + 1]].transpose(0, 1)[None].contiguous()
        vn = Vn[cu[b + 1] - keep:cu[b + 1]].transpose(0, 1)[None].contiguous()
        if page is None:
            fa.kv_cache_append(kn, vn, as_cache(Ku[b:b + 1]), as_cache(Vu[b:b + 1]), t32([lens[b]]), **ds)
        else:
            fa.kv_cache_append_paged(kn, vn, as_cache(Ku), as_cache(Vu), table[b:b + 1], t32([lens[b]]), **ds)
    torch.cuda.synchronize()
    return Kr, Vr, Ku, Vu, (Kn, Vn, table, ds)


SQ = [1, 0, 5, 16, 17, 64, 65, 130, 1, 40]


@pytest.mark.parametrize("fp8", [True, False])
@pytest.mark.parametrize("page", [None, 16, 128])
@pytest.mark.parametrize("d", [64, 128])
def test_the_ragged_append_writes_what_the_uniform_append_writes_per_sequence(d, page, fp8):
    """all four cache forms, a mixed batch: positions around the page and the 64-position boundaries (the uniform kernel's blocks),
    sq_b > L (sequence 7: 130 rows, 100 keys -- the leading 30 rows are dropped), L <= 0 (sequences 3 and 8), sq_b = 0 (sequence 1,
    with a garbage length), a length above the capacity (sequence 6)"""
    cap = 384
    lens = [129, 2 ** 31 - 1, 64, 0, 17, 127, cap + 7, 100, -5, 256 + 40]
    Kr, Vr, Ku, Vu, _ = both_ways(SQ, lens, cap, d, fp8, page, 200 + d)
    assert same(Kr, Ku) and same(Vr, Vu)
    untouched = sentinel(Kr.shape, fp8)
    assert not same(Kr, untouched) and not same(Vr, untouched), "nothing was written"


@pytest.mark.parametrize("page", [None, 16])
def test_against_the_cpu_writer(page):
    """one fp8 case against kv_append_check.append, sequence by sequence"""
    d, cap = 128, 256
    sq, lens = [3, 0, 70, 1], [3, 9, 200, 256]
    Kr, Vr, _, _, (Kn, Vn, table, ds) = both_ways(sq, lens, cap, d, True, page, 300)
    cu = cu_of(sq)
    wantK, wantV = sentinel(Kr.shape, True).cpu(), sentinel(Vr.shape, True).cpu()
    for b, s in enumerate(sq):
        if s == 0:
            continue
        kn, vn = (t[cu[b]:cu[b + 1]].transpose(0, 1)[None].cpu() for t in (Kn, Vn))
        if page is None:
            wantK[b:b + 1] = kc.append(kn, wantK[b:b + 1], [lens[b]], ds["k_descale"].cpu())
            wantV[b:b + 1] = kc.append(vn, wantV[b:b + 1], [lens[b]], ds["v_descale"].cpu())
        else:
            wantK = kc.append(kn, wantK, [lens[b]], ds["k_descale"].cpu(), table[b:b + 1].cpu())
            wantV = kc.append(vn, wantV, [lens[b]], ds["v_descale"].cpu(), table[b:b + 1].cpu())
    assert kc.same_bytes(Kr, wantK) and kc.same_bytes(Vr, wantV)


@pytest.mark.parametrize("fp8", [True, False])
def test_boundaries_one_row_and_many(fp8):
    """first positions at and around multiples of 16 (the page), 64 (the uniform kernel's block) and the end of the capacity"""
    d, cap, page = 64, 256, 16
    for s in (1, 3, 33):
        firsts = [0, 15, 16, 17, 63, 64, 65, 127, 128, cap - s]
        lens = [f + s for f in firsts]
        sq = [s] * len(firsts)
        for pg in (None, page):
            Kr, Vr, Ku, Vu, _ = both_ways(sq, lens, cap, d, fp8, pg, 400 + s)
            assert same(Kr, Ku) and same(Vr, Vu), (s, pg)


@pytest.mark.parametrize("fp8", [True, False])
def test_a_bad_table_entry_is_skipped_never_clamped(fp8):
    d, cap, page = 128, 128, 16
    sq, lens = [40, 20, 5], [100, 128, 5]
    B, n = 3, cap // page
    P = B * n + 4
    table = torch.randperm(P, generator=torch.Generator().manual_seed(7))[:B * n].reshape(B, n).to(i32)
    table[0, 4] = P            # positions 64 .. 79 of sequence 0: skipped
    table[0, 5] = -1           # positions 80 .. 95
    table[1, 7] = 2 ** 31 - 1  # positions 112 .. 127 of sequence 1
    table[2, 1:] = -2 ** 31    # pages sequence 2 does not reach: never read
    Kr, Vr, Ku, Vu, _ = both_ways(sq, lens, cap, d, fp8, page, 500, table=table)
    assert same(Kr, Ku) and same(Vr, Vu)
    # what was written: sequence 0's positions 60 .. 63 and 96 .. 99, nothing in between
    page_of = lambda b, p: int(table[b, p // page])
    sent = SENT[u8 if fp8 else i16]
    assert bool((Kr[page_of(0, 60), :, 60 % page:] != sent).any()) and bool((Kr[page_of(0, 96), :, :4] != sent).any())


@pytest.mark.parametrize("page", [None, 16])
def test_strided_new_rows(page):
    d, cap = 128, 256
    sq, lens = [7, 0, 50, 1], [7, 3, 250, 256]
    Kr, Vr, Ku, Vu, _ = both_ways(sq, lens, cap, d, True, page, 600, strided=True)
    Kd, Vd, _, _, _ = both_ways(sq, lens, cap, d, True, page, 600)
    assert same(Kr, Ku) and same(Vr, Vu) and same(Kr, Kd) and same(Vr, Vd)


def test_more_rows_than_the_capacity_and_many_sequences():
    """totalQ is not capped at the capacity: 70 sequences (the binary search crosses 64) bring 3 x the capacity in rows"""
    d, cap = 64, 32
    sq = [(3 * b) % 5 for b in range(69)] + [cap + 9]                    # the last sequence alone brings more rows than the capacity
    lens = [min(cap, 1 + (7 * b) % 40) for b in range(69)] + [cap]
    assert sum(sq) > 3 * cap
    for page in (None, 16):
        Kr, Vr, Ku, Vu, _ = both_ways(sq, lens, cap, d, True, page, 700)
        assert same(Kr, Ku) and same(Vr, Vu), page
