"""flash_attention_mla_prefill on the GPU against the float64 softmax under kv_cache_check.assert_close (1e-3 + 1e-3 |ref| on fp32 O, the
LSE bound).  The kernel's seams: 64-key tiles, 64-row waves, 256-row units, 1024 visible keys between the weight pair and single bf16."""
import pytest
import torch

from kv_cache_check import DEV, assert_close, fa, ratios, same_bits
from mla_prefill_check import DQK, DV, case, reference, run, visible

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (63, 63), (64, 64), (65, 65), (129, 129), (255, 255), (256, 256), (257, 257), (300, 300), (70, 333), (300, 40)]


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "model_layout"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Sq,Sk", SHAPES)
def test_parity(Sq, Sk, causal, strided):
    """every row sees fewer than 1024 keys: the pair form holds the stated tolerance on every element"""
    Q, K, V, (refO, refL, _) = case(2, 3, Sq, Sk, causal)
    O, lse = run(Q, K, V, causal, strided)
    assert_close(O, lse, refO, refL, f"mla_prefill {Sq}x{Sk} causal={causal} strided={strided}")


@pytest.mark.parametrize("Sq,Sk,causal,flagged", [(1280, 1280, True, False), (256, 1280, False, False), (300, 300, False, True)])
def test_single_weights_range(Sq, Sk, causal, flagged):
    """rows q < 1024 of the causal default call: the stated tolerance alone.  Every other row here has single bf16 weights and is held
    to 1e-3 + 1e-3 |ref| + 2^-9 sum_k p_k |v_k|: one bf16 rounding per weight under an unrounded normaliser, a derived bound"""
    Q, K, V, (refO, refL, absPV) = case(1, 2, Sq, Sk, causal)
    O, lse = run(Q, K, V, causal, weights_dtype=torch.bfloat16 if flagged else None)
    O, lse = O.double().cpu(), lse.double().cpu()
    assert torch.isfinite(O).all()
    r, lr = ratios(O, lse, refO, refL)
    wide = (O - refO).abs() / (1e-3 + 1e-3 * refO.abs() + 2.0 ** -9 * absPV)
    early = torch.arange(Sq) < (1024 if causal and not flagged else 0)
    print(f"{Sq}x{Sk}: early rows, worst error / tolerance {r[:, :, early].max().item() if early.any() else 0:.3f}; single-weight rows, "
          f"worst error / derived bound {wide[:, :, ~early].max().item():.3f} (/ bare tolerance {r[:, :, ~early].max().item():.3f})")
    assert (r[:, :, early] <= 1).all() and (wide[:, :, ~early] <= 1).all() and (lr <= 1).all()


@pytest.mark.parametrize("Sq,Sk,causal", [(129, 129, True), (70, 333, False)])
def test_count_probe(Sq, Sk, causal):
    """Q = 0: every weight is exactly 1, so the LSE counts the visible keys and O is the mean of the visible rows of an index-coded V
    (k + c / 128 rounded to bf16; the reference is taken on the rounded values): mask, zeroed ragged tail, tile count of every row"""
    B, H = 2, 3
    Q, K = torch.zeros(B, H, Sq, DQK, dtype=torch.bfloat16), torch.ones(B, H, Sk, DQK, dtype=torch.bfloat16)
    V = (torch.arange(Sk)[:, None] + torch.arange(DV)[None, :] / 128).to(torch.bfloat16).expand(B, H, Sk, DV).contiguous()
    O, lse = run(Q, K, V, causal)
    vis = visible(Sq, Sk, causal).double()
    n = vis.sum(-1)
    refL, refO = torch.log(n).expand(B, H, Sq), ((vis @ V[0, 0].double()) / n[:, None]).expand(B, H, Sq, DV)
    assert ((lse.double().cpu() - refL).abs() <= 2.0 ** -22 * refL.abs() + 1e-6).all()
    assert ((O.double().cpu() - refO).abs() <= 2.0 ** -20 * refO.abs()).all()


def test_output_types_lse_and_repeats():
    Q, K, V, _ = case(2, 3, 300, 300, True)
    O, lse = run(Q, K, V, True)
    for dt in (torch.bfloat16, torch.float16):
        assert same_bits(run(Q, K, V, True, out_dtype=dt)[0], O.to(dt)), dt   # fp32 O rounded once
    assert same_bits(fa.flash_attention_mla_prefill(Q.to(DEV), K.to(DEV), V.to(DEV), is_causal=True, out_dtype=torch.float32), O)
    O2, lse2 = run(Q, K, V, True)
    assert same_bits(O2, O) and same_bits(lse2, lse)


@pytest.mark.parametrize("key", [299, 10], ids=["beyond_early_diagonals", "inside"])
def test_huge_value(key):
    """one V entry of 1e30: finite everywhere, and the rows that do not see it (q < key under the mask) within the tolerance"""
    Q, K, V, _ = case(2, 3, 300, 300, True)
    V = V.clone()
    V[1, 2, key, 5] = 1e30
    refO, refL, _ = reference(Q, K, V, True)
    O, lse = run(Q, K, V, True)
    assert torch.isfinite(O).all() and torch.isfinite(lse).all()
    assert_close(O[:, :, :key], lse[:, :, :key], refO[:, :, :key], refL[:, :, :key], f"1e30 at key {key}")


def test_graph_replays():
    Q, K, V = (t.to(DEV) for t in case(2, 3, 300, 300, True)[:3])
    eager, eager_lse = fa.flash_attention_mla_prefill(Q, K, V, is_causal=True, out_dtype=torch.float32, return_lse=True)
    O, lse = torch.empty_like(eager), None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, lse = fa.flash_attention_mla_prefill(Q, K, V, O=O, is_causal=True, return_lse=True)
    for _ in range(2):
        O.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(O, eager) and same_bits(lse, eager_lse)
