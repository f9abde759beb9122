"""GPU tests of flash_attention_decode (split-KV decode): parity with the float64 explicit softmax over the visible keys of each
sequence (every element of the fp32 output within the stated 1e-3 + 1e-3 |ref|; the LSE within rtol 2e-6, atol 2e-4), the
bottom-right mask, per-sequence lengths read on the device, forced split counts (empty splits included), garbage beyond the length,
strided caches, determinism, graph replay with lengths that change in place, a side stream, and one test at serving size."""
import functools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

from kv_cache_check import CAP, DEV, assert_close, randn, reference  # noqa: E402

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


# (B, H, Hkv, Sq, capacity, kv_lens, causal)
SWEEP = [
    (2, 8, 2, 1, 64, [1, 64], False),                          # G 4; the smallest capacity; length 1; the full capacity
    (3, 8, 8, 2, 300, [2, 17, 300], True),                     # G 1; length = Sq; 17; capacity not a multiple of the tile
    (4, 16, 2, 5, 1024, [127, 128, 129, 1000], True),          # G 8, G * Sq = 40: three row blocks; one tile +- 1
    (2, 16, 1, 16, 512, [17, 333], True),                      # multi-query, G 16, Sq 16: sixteen row blocks
    (2, 32, 8, 1, 4096, None, False),                          # kv_lens = None
    (3, 8, 2, 16, 2048, [1, 16, 2048], True),                  # a length below Sq: rows that only see key 0
    (2, 8, 2, 1, 65536, [5, 65536], False),                    # very short beside very long
    (1, 16, 4, 2, 70000, [69999], True),                       # a capacity above 65 536, not a multiple of anything
    (2, 32, 2, 1, 640, [129, 640], True),                      # G 16, one row block exactly
    (3, 4, 4, 5, 256, [1, 5, 255], False),                     # no mask with several rows
]


@functools.lru_cache(maxsize=2)
def sweep_case(i, d):
    B, H, Hkv, Sq, cap, lens, causal = SWEEP[i]
    Q, K, V = randn((B, H, Sq, d), 100 + i, BF16), randn((B, Hkv, cap, d), 200 + i, BF16), randn((B, Hkv, cap, d), 300 + i, BF16)
    refO, refL = reference(Q, K, V, lens, causal)
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    return Q.to(DEV), K.to(DEV), V.to(DEV), lens_d, refO, refL


@pytest.mark.parametrize("splits", [0, 1, 2, 3, CAP])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("i", range(len(SWEEP)))
def test_sweep_against_float64(i, d, splits):
    B, H, Hkv, Sq, cap, lens, causal = SWEEP[i]
    Q, K, V, lens_d, refO, refL = sweep_case(i, d)
    plan = fa.decode_plan(B, H, Hkv, Sq, cap, d, fa.FA_DTYPE_F32, splits)
    assert plan["row_blocks"] == -(-(H // Hkv) * Sq // plan["rows_per_block"]) and (splits == 0 or plan["num_splits"] == splits)
    O, lse = fa.flash_attention_decode(Q, K, V, lens_d, is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True)
    torch.cuda.synchronize()
    assert_close(O, lse, refO, refL, f"case {i} d {d} splits {plan['num_splits']}")
    # bf16 / fp16 output: the fp32 result of the same call rounded once
    for dt in (torch.bfloat16, torch.float16):
        Ol = fa.flash_attention_decode(Q, K, V, lens_d, is_causal=causal, out_dtype=dt, num_splits=splits)
        assert Ol.dtype == dt and torch.equal(Ol, O.to(dt)), dt


@pytest.mark.parametrize("d", [64, 128])
def test_agrees_with_the_prefill_path_where_the_two_mean_the_same(d):
    """no mask, kv_lens = None: flash_attention() computes the same function (fp16 weights); both within the tolerance of float64"""
    B, H, Hkv, Sq, Sk = 2, 16, 4, 4, 2048
    Q, K, V = randn((B, H, Sq, d), 1, BF16), randn((B, Hkv, Sk, d), 2, BF16), randn((B, Hkv, Sk, d), 3, BF16)
    refO, refL = reference(Q, K, V, None, False)
    Qd, Kd, Vd = Q.to(DEV), K.to(DEV), V.to(DEV)
    O, lse = fa.flash_attention_decode(Qd, Kd, Vd, out_dtype=torch.float32, return_lse=True)
    P, plse = fa.flash_attention(Qd, Kd, Vd, out_dtype=torch.float32, return_lse=True, weights_dtype=torch.float16)
    torch.cuda.synchronize()
    assert_close(O, lse, refO, refL, "decode")
    assert_close(P, plse, refO, refL, "prefill")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_garbage_beyond_the_length_never_enters_the_result(d, causal):
    B, H, Hkv, Sq, cap = 3, 8, 2, 4, 1024
    lens = [1, 200, 1000]
    Q, K, V = randn((B, H, Sq, d), 11, BF16), randn((B, Hkv, cap, d), 12, BF16), randn((B, Hkv, cap, d), 13, BF16)
    Kz, Vz, Kg, Vg = K.clone(), V.clone(), K.clone(), V.clone()
    for b, L in enumerate(lens):
        Kz[b, :, L:], Vz[b, :, L:] = 0, 0
        Kg[b, :, L::2], Kg[b, :, L + 1::2] = float("nan"), 1e30
        Vg[b, :, L::2], Vg[b, :, L + 1::2] = 1e30, float("nan")
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for splits in (0, 1, 3, CAP):
        clean = fa.flash_attention_decode(Q.to(DEV), Kz.to(DEV), Vz.to(DEV), lens_d, is_causal=causal, out_dtype=torch.float32,
                                          num_splits=splits, return_lse=True)
        dirty = fa.flash_attention_decode(Q.to(DEV), Kg.to(DEV), Vg.to(DEV), lens_d, is_causal=causal, out_dtype=torch.float32,
                                          num_splits=splits, return_lse=True)
        torch.cuda.synchronize()
        assert torch.isfinite(dirty[0]).all() and torch.isfinite(dirty[1]).all()
        assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])
    if causal:
        # the keys the mask hides from row i (visible to later rows: finite data) do not reach row i either: huge values in the last
        # key, which only the last row sees, leave every other row bit for bit
        Kh, Vh = Kz.clone(), Vz.clone()
        for b, L in enumerate(lens):
            Kh[b, :, L - 1], Vh[b, :, L - 1] = 1e30, 1e30
        clean = fa.flash_attention_decode(Q.to(DEV), Kz.to(DEV), Vz.to(DEV), lens_d, is_causal=True, out_dtype=torch.float32,
                                          return_lse=True)
        hidden = fa.flash_attention_decode(Q.to(DEV), Kh.to(DEV), Vh.to(DEV), lens_d, is_causal=True, out_dtype=torch.float32,
                                           return_lse=True)
        torch.cuda.synchronize()
        rows = [b for b, L in enumerate(lens) if L >= Sq]   # (a length below Sq: every row sees key 0 = the last key)
        assert torch.equal(hidden[0][rows, :, :-1], clean[0][rows, :, :-1]) and torch.equal(hidden[1][rows, :, :-1], clean[1][rows, :, :-1])


@pytest.mark.parametrize("d", [64, 128])
def test_strided_views_of_model_layout_buffers(d):
    B, H, Hkv, Sq, cap = 2, 16, 4, 3, 777
    q = randn((B, Sq, H * d), 21, BF16).to(DEV)
    kc, vc = randn((B, cap, Hkv * d), 22, BF16).to(DEV), randn((B, cap, Hkv * d), 23, BF16).to(DEV)
    lens_d = torch.tensor([300, 777], dtype=torch.int32, device=DEV)
    view = lambda t, h: t.view(B, t.shape[1], h, d).transpose(1, 2)
    out = torch.zeros((B, Sq, H * d), dtype=torch.float32, device=DEV)
    Q, K, V = view(q, H), view(kc, Hkv), view(vc, Hkv)
    assert not K.is_contiguous()
    fa.flash_attention_decode(Q, K, V, lens_d, is_causal=True, O=view(out, H))
    dense = fa.flash_attention_decode(Q.contiguous(), K.contiguous(), V.contiguous(), lens_d, is_causal=True, out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(view(out, H), dense)
    refO, _ = reference(Q.cpu(), K.cpu(), V.cpu(), [300, 777], True)
    assert ((dense.double().cpu() - refO).abs() <= 1e-3 + 1e-3 * refO.abs()).all()


def test_deterministic_and_the_lse_request_leaves_o_alone():
    B, H, Hkv, Sq, cap, d = 4, 32, 8, 2, 8192, 128
    Q, K, V = randn((B, H, Sq, d), 31, BF16).to(DEV), randn((B, Hkv, cap, d), 32, BF16).to(DEV), randn((B, Hkv, cap, d), 33, BF16).to(DEV)
    lens_d = torch.tensor([8192, 100, 4097, 6000], dtype=torch.int32, device=DEV)
    for splits in (0, 1, 7):
        a = fa.flash_attention_decode(Q, K, V, lens_d, is_causal=True, num_splits=splits, out_dtype=torch.float32)
        b = fa.flash_attention_decode(Q, K, V, lens_d, is_causal=True, num_splits=splits, out_dtype=torch.float32)
        c, lse = fa.flash_attention_decode(Q, K, V, lens_d, is_causal=True, num_splits=splits, out_dtype=torch.float32, return_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and torch.isfinite(lse).all()


def test_graph_replay_reads_the_lengths_of_the_moment():
    """one captured call (a linear chain: split kernel, combine kernel); kv_lens and the cache change IN PLACE between replays"""
    B, H, Hkv, Sq, cap, d = 3, 16, 4, 1, 4096, 128
    Q, K, V = randn((B, H, Sq, d), 41, BF16).to(DEV), randn((B, Hkv, cap, d), 42, BF16).to(DEV), randn((B, Hkv, cap, d), 43, BF16).to(DEV)
    lens_d = torch.tensor([10, 1000, 4000], dtype=torch.int32, device=DEV)
    plan = fa.decode_plan(B, H, Hkv, Sq, cap, d, fa.FA_DTYPE_F32)
    assert plan["num_splits"] > 1
    ws = torch.empty(fa.decode_workspace_size(B, H, Sq, d, plan["num_splits"]), dtype=torch.uint8, device=DEV)
    O = torch.zeros((B, H, Sq, d), dtype=torch.float32, device=DEV)
    eager = lambda: fa.flash_attention_decode(Q, K, V, lens_d, is_causal=True, out_dtype=torch.float32).clone()
    fa.flash_attention_decode(Q, K, V, lens_d, is_causal=True, O=O, workspace=ws)   # (first call outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.flash_attention_decode(Q, K, V, lens_d, is_causal=True, O=O, workspace=ws)
    O.zero_()
    graph.replay()
    torch.cuda.synchronize()
    first = eager()
    assert torch.equal(O, first)
    # one decode step later: a new row appended to every sequence's cache, the lengths advanced, all in place
    for b, L in enumerate([10, 1000, 4000]):
        K[b, :, L], V[b, :, L] = randn((Hkv, d), 44 + b, BF16).to(DEV), randn((Hkv, d), 47 + b, BF16).to(DEV)
    lens_d += 1
    lens_d[0] = 3000
    graph.replay()
    torch.cuda.synchronize()
    second = eager()
    assert torch.equal(O, second) and not torch.equal(first, second)
    refO, _ = reference(Q.cpu(), K.cpu(), V.cpu(), [3000, 1001, 4001], True)
    assert ((O.double().cpu() - refO).abs() <= 1e-3 + 1e-3 * refO.abs()).all()


def test_decode_on_a_side_stream_keeps_its_workspace():
    """stream=: the kernels run on a side stream while the current stream goes on allocating blocks of the workspace's size and
    overwriting them; the workspace released at return must not be one of them while the kernels still use it"""
    B, H, Hkv, Sq, cap, d = 8, 32, 8, 4, 16384, 128
    Q, K, V = randn((B, H, Sq, d), 51, BF16).to(DEV), randn((B, Hkv, cap, d), 52, BF16).to(DEV), randn((B, Hkv, cap, d), 53, BF16).to(DEV)
    ns = fa.decode_plan(B, H, Hkv, Sq, cap, d, fa.FA_DTYPE_F32)["num_splits"]
    n = fa.decode_workspace_size(B, H, Sq, d, ns)
    assert ns > 1 and n > 0
    ref = fa.flash_attention_decode(Q, K, V, out_dtype=torch.float32)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(3):
        got = fa.flash_attention_decode(Q, K, V, out_dtype=torch.float32, stream=side)
        junk = [torch.full((n,), 255, dtype=torch.uint8, device=DEV) for _ in range(4)]   # NaN bytes, on the current stream
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(got, ref)
        del junk, got


def test_at_serving_size_sampled_heads_against_float64():
    B, H, Hkv, Sq, cap, d = 4, 64, 8, 1, 131072, 128
    lens = [131072, 77, 50001, 100000]
    g = torch.Generator(device=DEV).manual_seed(61)
    Q = torch.randn((B, H, Sq, d), generator=g, device=DEV).bfloat16()
    K = torch.randn((B, Hkv, cap, d), generator=g, device=DEV).bfloat16()
    V = torch.randn((B, Hkv, cap, d), generator=g, device=DEV).bfloat16()
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    O, lse = fa.flash_attention_decode(Q, K, V, lens_d, is_causal=True, out_dtype=torch.float32, return_lse=True)
    torch.cuda.synchronize()
    assert torch.isfinite(O).all()
    for b, kvh in ((0, 0), (1, 3), (2, 7), (3, 5)):
        hs = slice(kvh * 8, kvh * 8 + 8)
        refO, refL = reference(Q[b:b + 1, hs].cpu(), K[b:b + 1, kvh:kvh + 1].cpu(), V[b:b + 1, kvh:kvh + 1].cpu(), [lens[b]], True)
        assert_close(O[b:b + 1, hs], lse[b:b + 1, hs], refO, refL, f"batch {b} K/V head {kvh}")
