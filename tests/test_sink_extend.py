"""GPU tests of attention sinks in chunked prefill against the K/V caches, uniform and ragged (the flash_attention_extend* fronts with
``sinks=``: flash_attention_sink_extend, _extend_paged, _extend_varlen, _extend_paged_varlen).  Every case: B = 2, Hkv = 2, capacity 384
(three 128-key tiles); the reference, the sink vector and the runners shared with test_sink.py are in sink_check.py.

1. parity against the float64 reference (kv_cache_check.assert_close, unchanged) over d, G, both masks, windows 0 / 7 / 130, splits 1 / 3 /
   the library's choice, the four cache forms, fp32 and bf16 O; Sq 17 / 40 / 130 (G Sq = 68 is no multiple of a row block: blocks
   straddle heads with different sinks); ragged rows (5, 130), (17, 40) and (0, 40): an idle sequence
2. sinks = -inf everywhere: the bits of the call without sinks -- at window 0 also the WINDOW = true kernel against the WINDOW = false one
3. the exact probe: Q = 0, sinks = 0, window = 1 -- O is exactly half of one named key's V row, LSE = ln 2
4. sinks of +1e4, -1e4, +-80
5. the bit-equality contracts with sinks: paged = contiguous; Sq <= 16 chunked prefill = decode under the same forced splits; a ragged
   sequence = the uniform call on that sequence alone; poison beyond the length and below the window
6. a captured `kv_lens += Sq; append; extend with sinks` on a paged fp8 cache, replayed with the sinks tensor overwritten in between
7. a call with sinks fetches [the plan, the workspace size, flash_attention_sink_*]
"""
import itertools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import kv_cache_check as kv  # noqa: E402
import sink_check as sc  # noqa: E402
from kv_cache_check import DEV  # noqa: E402
from sink_check import FORM_IDS, FORMS  # noqa: E402

pytestmark = pytest.mark.gpu
ROWS = {"extend": (17, 40, 130), "varlen": ((5, 130), (17, 40), (0, 40))}
F32 = torch.float32


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("family", ["extend", "varlen"])
def test_parity_against_the_float64_reference(family, d, G, form):
    sc.run_parity(family, d, G, form, ROWS[family])


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("family,d,G,rows", [("extend", 64, 4, 17), ("extend", 128, 1, 130), ("varlen", 64, 1, (5, 130)),
                                             ("varlen", 128, 4, (0, 40))])
def test_sinks_of_minus_infinity_are_the_call_without_sinks_bit_for_bit(family, d, G, rows, form):
    sc.run_neg_inf(family, d, G, form, rows)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("d,G", [(64, 4), (128, 1)])
def test_exact_probe_half_of_one_named_key(d, G, form):
    sc.run_probe("extend", d, G, form, True, 40, ((1, 128), (129, 300)), (1, 3))
    sc.run_probe("extend", d, G, form, False, 1, ((1, 129), (300, 129)), (1,))
    sc.run_probe("varlen", d, G, form, True, (17, 40), ((1, 128), (129, 300)), (1, 3))
    sc.run_probe("varlen", d, G, form, False, (1, 1), ((1, 129), (300, 129)), (1,))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("family,d,G,rows", [("extend", 64, 4, 40), ("extend", 128, 1, 17), ("varlen", 128, 4, (5, 130)),
                                             ("varlen", 64, 1, (0, 40))])
def test_range_of_the_sink(family, d, G, rows, form):
    sc.run_range(family, d, G, form, rows)


@pytest.mark.parametrize("page,fp8", [(16, False), (128, True)])
@pytest.mark.parametrize("family,rows", [("extend", 40), ("varlen", (17, 40))])
@pytest.mark.parametrize("d", [64, 128])
def test_paged_equals_contiguous_on_the_same_bytes(d, family, rows, page, fp8):
    sc.run_paged_equal(family, d, rows, page, fp8, 1110 + d)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("d", [64, 128])
def test_sixteen_rows_or_fewer_are_decode_bit_for_bit(d, form):
    G = 4
    cache = kv.Cache(d, *form, 1120 + d)
    c = cache.device()
    sinks = sc.sinks_for(sc.HKV * G).to(DEV)
    for Sq in (1, 5, 16):
        Q = sc.queries("extend", d, G, Sq, 1121 + Sq).to(DEV)
        for lens, causal, W, ns in itertools.product(sc.LENS, (False, True), (0, 7, 130), (1, 3)):
            kw = dict(is_causal=causal, window=W, num_splits=ns, sinks=sinks, out_dtype=F32)
            a, b = kv.attend("extend", c, Q, kv.i32(lens), **kw), kv.attend("decode", c, Q, kv.i32(lens), **kw)
            assert kv.same_bits(a[0], b[0]) and kv.same_bits(a[1], b[1]), (Sq, lens, causal, W, ns)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("d", [64, 128])
def test_a_ragged_sequence_is_the_uniform_call_on_that_sequence_alone(d, form):
    G = 4
    page, fp8 = form
    cache = kv.Cache(d, page, fp8, 1130 + d)
    c = cache.device()
    sinks = sc.sinks_for(sc.HKV * G).to(DEV)
    for rows in ROWS["varlen"]:
        Q = sc.queries("varlen", d, G, rows, 1131 + sum(rows)).to(DEV)
        cu = kv.cu_of(rows)
        for lens, causal, W, ns in itertools.product(sc.LENS, (False, True), (0, 130), (1, 3)):
            kw = dict(is_causal=causal, window=W, num_splits=ns, sinks=sinks, out_dtype=F32)
            O, lse = kv.attend("varlen", c, Q, kv.i32(lens), kv.i32(cu), **kw)
            for b, sq in enumerate(rows):
                if sq == 0:
                    continue
                # the sequence alone: a batch of one on its own slice of the cache (paged: its own row of the table)
                one = dict(c, K=c["K"] if page else c["K"][b:b + 1], V=c["V"] if page else c["V"][b:b + 1],
                           table=c["table"][b:b + 1] if page else None)
                Qb = Q[cu[b]:cu[b + 1]].transpose(0, 1)[None]
                Ob, lb = kv.attend("extend", one, Qb, kv.i32(lens[b:b + 1]), **kw)
                assert kv.same_bits(O[cu[b]:cu[b + 1]].transpose(0, 1), Ob[0]) and kv.same_bits(lse[:, cu[b]:cu[b + 1]], lb[0]), \
                    (rows, b, lens, causal, W, ns)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("family,rows", [("extend", 40), ("varlen", (17, 40))])
def test_poison_beyond_the_length_and_below_the_window_changes_no_bit(family, rows, form):
    sc.run_poison(family, 128, rows, form, 1140)


@pytest.mark.parametrize("ns", [1, 3])
def test_graph_replays_see_the_sinks_of_the_moment(ns):
    """`kv_lens += Sq; kv_cache_append_paged; flash_attention_extend_paged(sinks=)` on a page-16 fp8 cache (sink_check.run_graph); the
    reference reads the cache as it then is, dequantised"""
    d, G, Sq, start = 128, 4, 20, (100, 290)
    H = sc.HKV * G
    cache = kv.Cache(d, 16, True, 1150)
    c = cache.device()
    K, V, table, ds = c["K"], c["V"], c["table"], c["ds"]
    Qc = sc.queries("extend", d, G, Sq, 1151)
    Q = Qc.to(DEV)
    Kn, Vn = (sc.queries("extend", d, 1, Sq, 1152 + i).to(DEV) for i in range(2))       # [B, HKV, Sq, d]: the new rows
    lens, sinks = kv.i32(start), torch.zeros(H, dtype=torch.float32, device=DEV)
    O = torch.empty((sc.B, H, Sq, d), dtype=torch.float32, device=DEV)
    ws = torch.empty(max(fa.decode_workspace_size(sc.B, H, Sq, d, ns), 16), dtype=torch.uint8, device=DEV)

    def step():
        lens.add_(Sq)
        fa.kv_cache_append_paged(Kn, Vn, K, V, table, lens, **ds)
        return fa.flash_attention_extend_paged(Q, K, V, table, lens, is_causal=True, num_splits=ns, O=O, workspace=ws, return_lse=True,
                                               sinks=sinks, **ds)

    def reference(now, vec):
        K64, V64 = (kv.gather(kv.dequantise(T.cpu().view(torch.uint8), s), table.cpu()) for T, s in ((K, cache.kd), (V, cache.vd)))
        return sc.reference_sinks(Qc, K64, V64, now, True, 0, vec)[:2]

    sc.run_graph(step, lens, start, Sq, sinks, reference, O)


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("front,window", [("extend", None), ("extend_window", None), ("extend_window", 40)])
@pytest.mark.parametrize("family", ["extend", "varlen"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_a_call_with_sinks_fetches_the_plan_the_workspace_size_and_the_sink_entry_point(monkeypatch, form, family, front, window, ns):
    d, G = 64, 4
    rows = (3, 20) if family == "varlen" else 20
    c = kv.Cache(d, *form, 1160).device()
    paged, ragged = form[0] is not None, family == "varlen"
    mid = ("_paged" if paged else "") + ("_varlen" if ragged else "")
    args = [sc.queries(family, d, G, rows, 1161).to(DEV), c["K"], c["V"]] + ([c["table"]] if paged else []) \
        + ([kv.i32(kv.cu_of(rows))] if ragged else []) + [kv.i32((200, 256))]
    kw = dict(c["ds"], is_causal=True, num_splits=ns, **(dict(window=window) if front == "extend_window" else {}))
    sc.run_routing(monkeypatch, "flash_attention_extend" + mid + ("_window" if front == "extend_window" else ""), args, kw,
                   sc.sinks_for(sc.HKV * G).to(DEV), "flash_attention_extend" + ("_varlen" if ragged else "") + "_plan" + ("_window" if window else ""),
                   "flash_attention_sink_extend" + mid)
