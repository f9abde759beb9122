"""GPU tests of attention sinks in split-KV decode (flash_attention_decode / _paged with ``sinks=``: flash_attention_sink_decode,
flash_attention_sink_decode_paged).  Every case: B = 2, Hkv = 2, capacity 384 (three 128-key tiles); the reference, the sink vector and the
runners shared with test_sink_extend.py are in sink_check.py.

1. parity against the float64 reference (kv_cache_check.assert_close, unchanged) over d, G, both masks, windows 0 / 7 / 130, splits 1 / 3 /
   the library's choice, the four cache forms, fp32 and bf16 O; Sq 1 / 5 / 16, lengths (1, 300) and (129, 300)
2. sinks = -inf everywhere: the bits of the call without sinks
3. the exact probe: Q = 0, sinks = 0, window = 1 -- O is exactly half of one named key's V row, LSE = ln 2
4. sinks of +1e4, -1e4, +-80: finite, O = 0 and LSE = the sink for +1e4, the call without sinks for -1e4
5. the bit-equality contracts with sinks: paged = contiguous on the same bytes; poison beyond the length and below the window
6. a captured `kv_lens += Sq; append; decode with sinks`, replayed with the sinks tensor overwritten in between
7. a call with sinks fetches [the plan, the workspace size, flash_attention_sink_*]
"""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import kv_cache_check as kv  # noqa: E402
import sink_check as sc  # noqa: E402
from kv_cache_check import DEV  # noqa: E402
from sink_check import FORM_IDS, FORMS  # noqa: E402

pytestmark = pytest.mark.gpu
ROWS = (1, 5, 16)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("d", [64, 128])
def test_parity_against_the_float64_reference(d, G, form):
    sc.run_parity("decode", d, G, form, ROWS)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("d,G,Sq", [(64, 4, 5), (128, 1, 16), (128, 4, 1)])
def test_sinks_of_minus_infinity_are_the_call_without_sinks_bit_for_bit(d, G, Sq, form):
    sc.run_neg_inf("decode", d, G, form, Sq)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("d,G", [(64, 4), (128, 1)])
def test_exact_probe_half_of_one_named_key(d, G, form):
    sc.run_probe("decode", d, G, form, True, 5, ((1, 128), (129, 300)), (1, 3))
    sc.run_probe("decode", d, G, form, False, 1, ((1, 129), (300, 129)), (1,))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("d,G", [(64, 4), (128, 1)])
def test_range_of_the_sink(d, G, form):
    sc.run_range("decode", d, G, form, 5)


@pytest.mark.parametrize("page,fp8", [(16, False), (128, True)])
@pytest.mark.parametrize("d", [64, 128])
def test_paged_equals_contiguous_on_the_same_bytes(d, page, fp8):
    sc.run_paged_equal("decode", d, 5, page, fp8, 1010 + d)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_poison_beyond_the_length_and_below_the_window_changes_no_bit(form):
    sc.run_poison("decode", 64, 5, form, 1020)


@pytest.mark.parametrize("ns", [1, 3])
def test_graph_replays_see_the_sinks_of_the_moment(ns):
    """`kv_lens += Sq; kv_cache_append; flash_attention_decode(sinks=)` on a contiguous bf16 cache (sink_check.run_graph)"""
    d, G, Sq, W, start = 64, 4, 5, 130, (100, 290)
    H = sc.HKV * G
    cache = kv.Cache(d, None, False, 1030)
    K, V = cache.cK.to(DEV), cache.cV.to(DEV)
    Qc = sc.queries("decode", d, G, Sq, 1031)
    Q = Qc.to(DEV)
    Kn, Vn = (sc.queries("decode", d, 1, Sq, 1032 + i).to(DEV) for i in range(2))       # [B, HKV, Sq, d]: the new rows
    lens, sinks = kv.i32(start), torch.zeros(H, dtype=torch.float32, device=DEV)
    O = torch.empty((sc.B, H, Sq, d), dtype=torch.float32, device=DEV)
    ws = torch.empty(max(fa.decode_workspace_size(sc.B, H, Sq, d, ns), 16), dtype=torch.uint8, device=DEV)

    def step():
        lens.add_(Sq)
        fa.kv_cache_append(Kn, Vn, K, V, lens)
        return fa.flash_attention_decode(Q, K, V, lens, is_causal=True, window=W, num_splits=ns, O=O, workspace=ws, return_lse=True, sinks=sinks)

    sc.run_graph(step, lens, start, Sq, sinks, lambda now, vec: sc.reference_sinks(Qc, K.cpu(), V.cpu(), now, True, W, vec)[:2], O)


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("window", [None, 40])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_a_call_with_sinks_fetches_the_plan_the_workspace_size_and_the_sink_entry_point(monkeypatch, form, window, ns):
    d, G, Sq = 64, 4, 3
    c = kv.Cache(d, *form, 1040).device()
    paged = form[0] is not None
    args = [sc.queries("decode", d, G, Sq, 1041).to(DEV), c["K"], c["V"]] + ([c["table"]] if paged else []) + [kv.i32((200, 256))]
    sc.run_routing(monkeypatch, "flash_attention_decode" + ("_paged" if paged else ""), args,
                   dict(c["ds"], is_causal=True, window=window, num_splits=ns), sc.sinks_for(sc.HKV * G).to(DEV),
                   "flash_attention_decode_plan_window" if window else "flash_attention_decode_plan",
                   "flash_attention_sink_decode_paged" if paged else "flash_attention_sink_decode")
