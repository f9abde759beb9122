"""GPU: three memory rules of include/flash_attention.h that every call must keep, run on every kernel family.

  alignment   a base pointer needs 16 bytes and nothing more; kvLens, block tables, cu_seqlens_q and descales need 4
  workspace   its contents on entry are ignored, and it is exactly as large as the size function says
  bounds      a call writes O, the LSE, the gradients, the caches and its workspace, and nothing else

Every case runs once on plain torch allocations (zeroed outputs and workspace: the run the parity tests pin) and then with EVERY tensor
carved out of one arena of 0xFF bytes (tests/arena.py; tests/test_arena.py proves it on the CPU) -- outputs and workspace enter as
NaNs, the workspace at exactly its stated size, every tensor between untouched bands.  The two results must be equal bit for bit, the
arena must be untouched outside the outputs, and the inputs unchanged.  Two placements, in this order: `aligned` (everything at 0 mod
512: a difference can only come from the workspace contents or a store out of bounds) and `offset` (tensors at 16 mod 256, side inputs
at 4 mod 16: a difference that shows only here is an address formed wrongly).  The route is asserted through plan_ex / the decode
plans, and each arena result is also held to the suite's float64 references with their own bounds (weight_probe.forward_truth,
kv_cache_check.assert_close, grad_check.assert_grads, kv_append_check.append): no new tolerance."""
import functools
import math

import numpy as np
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import arena as ar  # noqa: E402
import kv_cache_check as kv  # noqa: E402
import grad_check as gc  # noqa: E402
import memory_contract as mc  # noqa: E402
import weight_probe as wp  # noqa: E402
from memory_contract import DEV, bf, f32  # noqa: E402

pytestmark = pytest.mark.gpu
FA_ERR_MISALIGNED = -2


def both_placements(call, judge, what, placements=mc.PLACEMENTS):
    """the pattern of every case: plain, then each placement -- bitwise equal to plain, arena clean, `judge(views)` against float64"""
    _, plain = mc.run(call, None)
    for placement in placements:
        arena, got = mc.run(call, placement)
        for n in call.outs:
            assert mc.same(got[n], plain[n]), f"{what} [{placement}]: {n} differs from the run on plain allocations"
        arena.check()
        if judge is not None:
            judge(got, f"{what} [{placement}]")
    return plain


# ---- a. forward -------------------------------------------------------------------------------------------------------------------
# wp.FORWARD runs d = 128 (80 and 136 where the family asks for it); the d = 64 instantiations, the other padded widths and the
# fp32 generic kernel are reached by these, built and judged by the same helpers (H = 64 at Sq = 1280: the smallest round head count
# on the persistent causal route at d = 64)
FORWARD_D64 = [
    wp.FwdCase("bf16_d64", "bf16", bf, f32, 32, 32, 1280, 1152, 64, False),
    wp.FwdCase("causal_mix_d64", "causal_mix", bf, bf, 64, 64, 1280, 1280, 64, True),
    wp.FwdCase("pair_d64", "pair", bf, f32, 8, 8, 600, 600, 64, True),
    wp.FwdCase("pair_d64_gqa_nc", "pair", bf, bf, 8, 2, 300, 700, 64, False),
    wp.FwdCase("bf16_padded_d40", "bf16_padded", bf, f32, 8, 8, 512, 700, 40, True),
    wp.FwdCase("fp8_d64", "fp8", "fp8", f32, 8, 8, 512, 512, 64, True),
    wp.FwdCase("f32_d64", "f32", f32, f32, 8, 8, 300, 300, 64, True),
    wp.FwdCase("f32_padded_d36", "f32", f32, f32, 8, 8, 300, 300, 36, False),
    wp.FwdCase("generic_f32_d256", "generic", f32, f32, 4, 4, 150, 150, 256, True),
]
FORWARD_CASES = dict(wp.FORWARD_BY_NAME, **{c.name: c for c in FORWARD_D64})


@functools.lru_cache(maxsize=None)
def forward_case(name):
    c = FORWARD_CASES[name]
    p = wp.build_forward(c)          # asserts the family through plan_ex
    return c, p, wp.forward_truth(c, p)


def judge_forward(c, p, t):
    def judge(v, what):
        worst, pair = wp.report(what, wp.ratios(v["O"].double().cpu(), t["O"], t["bound"]), [p["w0"]], c.H // c.Hkv)
        assert worst <= 1.0, f"{what}: pair (batch, head, q, k) = {pair} at {worst:.3g} x the bound"
        if c.lse:
            lse = v["lse"].double().cpu()
            assert torch.isfinite(lse).all() and ((lse - t["lse"]).abs() / t["lse_bound"]).max().item() <= 1.0, what
    return judge


@pytest.mark.parametrize("name", list(FORWARD_CASES))
def test_forward_every_family(name):
    c, p, t = forward_case(name)
    both_placements(mc.forward_call(c, p), judge_forward(c, p, t), f"forward {name} ({c.fam})")


@pytest.mark.parametrize("only", ["Q", "K", "V", "O", "lse"])
def test_forward_persistent_causal_one_tensor_shifted(only):
    """the persistent causal d = 128 kernel with one of its five tensors at 16 mod 256 and the other four at 0 mod 512: which side an
    address bug is on"""
    c, p, t = forward_case("causal_mix")
    assert c.d == 128 and c.causal and c.lse and c.fam == "causal_mix"
    both_placements(mc.forward_call(c, p), judge_forward(c, p, t), f"forward causal_mix, {only} alone shifted", [("only", only)])


@pytest.mark.parametrize("d,dtype", [(128, bf), (256, f32)])
def test_attention_weights(d, dtype):
    """flash_attention_weights (Q, K, LSE, P): the criteria of tests/test_flash_attention.py's attention-matrix tests"""
    B, H, Sq, Sk = 1, 2, 70, 150
    Q, K, V = (mc.randn((B, H, S, d), 50 + i, dtype) for i, S in enumerate((Sq, Sk, Sk)))
    for causal in (False, True):
        O, lse = fa.flash_attention(Q.to(DEV), K.to(DEV), V.to(DEV), is_causal=causal, out_dtype=f32, return_lse=True)
        torch.cuda.synchronize()
        s = Q.double().numpy() @ K.double().numpy().swapaxes(-1, -2) / np.sqrt(d)
        hidden = np.triu(np.ones((Sq, Sk), dtype=bool), 1)
        if causal:
            s = np.where(hidden, -np.inf, s)
        ref = np.exp(s - s.max(-1, keepdims=True))
        ref /= ref.sum(-1, keepdims=True)

        def judge(v, what):
            P = v["P"].cpu().numpy()
            if dtype == bf:
                np.testing.assert_allclose(P, ref, rtol=3e-3, atol=1e-6, err_msg=what)    # the LSE carries the bf16-P row-sum error
            else:
                np.testing.assert_allclose(P.sum(-1), 1.0, atol=2e-5, err_msg=what)
                Oc = O.cpu().numpy()                                                      # P V reproduces the fused kernel's O
                assert (np.abs(P @ V.numpy() - Oc) <= 2e-5 + 1e-4 * np.abs(Oc)).all(), what
            assert not causal or (P[..., hidden] == 0).all(), what

        both_placements(mc.weights_call(Q, K, lse.cpu(), causal), judge, f"weights d {d} causal {causal}")


# ---- b. backward ------------------------------------------------------------------------------------------------------------------
BWD_SHAPES = [(77, 77), (300, 300), (100, 500), (1, 500)]
BWD_DTYPES = [(f32, f32), (bf, bf), (f32, bf), (bf, f32)]


def backward_inputs(B, H, Hkv, Sq, Sk, d, seed):
    return (mc.randn((B, H, Sq, d), seed), mc.randn((B, Hkv, Sk, d), seed + 1), mc.randn((B, Hkv, Sk, d), seed + 2),
            mc.randn((B, H, Sq, d), seed + 3))


def judge_backward(Q, K, V, dO, causal, o_dtype):
    scale = 1.0 / math.sqrt(Q.shape[-1])
    g = dO.to(o_dtype)
    ref, _ = gc.reference_grads(Q, K, V, scale, causal, dO=g)
    mag = gc.magnitudes(Q, K, V, g, scale, causal)
    return lambda v, what: gc.assert_grads([v[n].double().cpu() for n in ("dQ", "dK", "dV")], ref, mag, what)


def backward_case(call, judge, what):
    """Sk <= 512: at most two 256-key blocks add into an element of dQ, onto a +0 that bwd_pre_kernel wrote; a sum of two terms onto
    +0 does not depend on their order, so dQ is reproducible bit for bit like dK and dV.  Asserted here before it is relied on"""
    _, one = mc.run(call, None)
    _, two = mc.run(call, None)
    for n in call.outs:
        assert mc.same(one[n], two[n]), f"{what}: two plain runs differ in {n}: the shape is not bit-reproducible"
    both_placements(call, judge, what)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_backward(d, causal):
    """the three backward kernels: ragged tail slices (Sq no multiple of 32), ragged tail keys (Sk no multiple of 64 or 256), one and
    two key blocks, H = 4 over Hkv = 4 and 1, every (O / dO, gradient) type pair; the workspace of exactly
    flash_attention_backward_workspace_size bytes enters full of NaNs"""
    B, H = 2, 4
    for si, (Sq, Sk) in enumerate(BWD_SHAPES):
        for hi, Hkv in enumerate((4, 1)):
            o_dtype, grad_dtype = BWD_DTYPES[(si + hi + 2 * causal + (d == 128)) % 4]
            Q, K, V, dO = backward_inputs(B, H, Hkv, Sq, Sk, d, 1000 * si + 10 * d + causal + 100 * hi)
            call = mc.backward_call(Q, K, V, dO, causal, o_dtype, grad_dtype)
            assert call.ws_bytes == fa.backward_workspace_size(B, H, Sq, d) > 0
            backward_case(call, judge_backward(Q, K, V, dO, causal, o_dtype),
                          f"backward d {d} causal {causal} {Sq}x{Sk} Hkv {Hkv} O {o_dtype} grads {grad_dtype}")


@pytest.mark.parametrize("d", [64, 128])
def test_backward_model_layout(d):
    """all nine tensors as [1, H, S, d] views of (1, S, H * d) buffers"""
    H, Hkv, Sq, Sk = 4, 2, 100, 300
    Q, K, V, dO = backward_inputs(1, H, Hkv, Sq, Sk, d, 7000 + d)
    call = mc.backward_call(Q, K, V, dO, True, f32, f32, layout="model")
    assert all(call.specs[n]["strides"] is not None for n in ("Q", "K", "V", "O", "dO", "dQ", "dK", "dV"))
    backward_case(call, judge_backward(Q, K, V, dO, True, f32), f"backward model layout d {d}")


# ---- c. split-KV: decode, extend, ragged ------------------------------------------------------------------------------------------
LENS = [1, 129, 300]                           # uniform calls: one sequence per length
ROWS = {"decode": (1, 5), "extend": (17, 130)}  # with G = 4: 20 packed rows (no multiple of 16); rows across one and several row blocks
RAGGED_ROWS, RAGGED_LENS, UNOWNED = [5, 0, 130, 17], [129, -5, 300, 1], 23       # an idle slot (its length is garbage); 17 rows on 1 key
WINDOWS, SPLITS = (0, 100), (1, 3, 8)          # 8 splits: more than the tiles of the short sequences, so some come out empty


@functools.lru_cache(maxsize=None)
def cache_of(B, d, page, fp8):
    return mc.Cache(B, d, page, fp8, seed=500 + d + (page or 0) + 7 * fp8)


def judge_uniform(cache, Q, causal, W):
    refO, refL = kv.reference(Q, cache.refK, cache.refV, LENS, causal, W)
    return lambda v, what: kv.assert_close(v["O"], v["lse"], refO, refL, what)


def rounded_once(plain32):
    """judge of a bf16-output call: the fp32 result of the same call (held to float64 above) rounded once, and the same LSE"""
    def judge(v, what):
        assert torch.equal(v["O"], plain32["O"].to(bf)) and mc.same(v["lse"], plain32["lse"]), f"{what}: not the fp32 result rounded once"
    return judge


@pytest.mark.parametrize("page,fp8", mc.FORMS)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("family", ["decode", "extend"])
def test_split_kv_uniform(family, d, page, fp8):
    cache = cache_of(len(LENS), d, page, fp8)
    for si, Sq in enumerate(ROWS[family]):
        Q = mc.randn((len(LENS), mc.HKV * mc.G, Sq, d), 600 + Sq)
        for W in WINDOWS:
            causal = bool((si + (W > 0)) % 2 == 0)             # both masks with and without a window
            judge = judge_uniform(cache, Q, causal, W)
            for ns in SPLITS:
                call = mc.split_kv_call(family, cache, Q, LENS, causal, ns, W)
                assert call.ws_bytes == fa.decode_workspace_size(len(LENS), mc.HKV * mc.G, Sq, d, ns) and (call.ws_bytes > 0) == (ns > 1)
                plain = both_placements(call, judge, call.note)
                # a bf16 O is the fp32 O of the same call rounded once, at the store (2-byte elements: other addresses behind the same base)
                rounded = mc.split_kv_call(family, cache, Q, LENS, causal, ns, W, odt=bf)
                both_placements(rounded, rounded_once(plain), rounded.note)


@pytest.mark.parametrize("page,fp8", mc.FORMS)
@pytest.mark.parametrize("d", [64, 128])
def test_split_kv_ragged(d, page, fp8):
    """rows (5, 0, 130, 17) and 23 rows behind them that no sequence owns: those must come back as the 0xFF they went in as"""
    B, H = len(RAGGED_ROWS), mc.HKV * mc.G
    cache = cache_of(B, d, page, fp8)
    cu = kv.cu_of(RAGGED_ROWS)
    T = cu[-1] + UNOWNED
    Q = mc.randn((T, H, d), 700 + d)
    for W in WINDOWS:
        causal = W == 0
        refO, refL, owned = kv.reference_ragged(Q, cache.refK, cache.refV, RAGGED_ROWS, RAGGED_LENS, causal, W)
        assert int(owned.sum()) == cu[-1] and not bool(owned[cu[-1]:].any())

        def judge(v, what):
            O, lse = v["O"].cpu(), v["lse"].cpu()
            kv.assert_close(O[owned], lse[:, owned], refO[owned], refL[:, owned], what)
            assert bool((O[~owned].view(torch.int32) == -1).all()) and bool((lse[:, ~owned].view(torch.int32) == -1).all()), \
                f"{what}: a row that no sequence owns was written"

        for ns in SPLITS:
            call = mc.split_kv_call("varlen", cache, Q, RAGGED_LENS, causal, ns, W, cu=cu)
            assert call.ws_bytes == fa.decode_workspace_size(1, H, T, d, ns)
            _, plain = mc.run(call, None)
            for placement in mc.PLACEMENTS:
                arena, got = mc.run(call, placement)
                assert mc.same(got["O"][:cu[-1]], plain["O"][:cu[-1]]) and mc.same(got["lse"][:, :cu[-1]], plain["lse"][:, :cu[-1]]), \
                    f"{call.note} [{placement}]: differs from the run on plain allocations"
                assert not plain["O"][cu[-1]:].any() and not plain["lse"][:, cu[-1]:].any()
                arena.check()
                judge(got, f"{call.note} [{placement}]")


# ---- d. cache append --------------------------------------------------------------------------------------------------------------
APPEND_ROWS, APPEND_LENS = 5, [5, 129, 300, 3]      # the first rows of a cache, rows across a tile and page seam, more rows than keys


@pytest.mark.parametrize("page,fp8", [(None, False), (None, True), (16, False), (128, True)])
@pytest.mark.parametrize("ragged", [False, True])
def test_cache_append(ragged, page, fp8):
    """both append kernels: the whole cache afterwards is the plain run's and kv_append_check.append's, byte for byte"""
    d, B = 128 if fp8 else 64, 4
    base = cache_of(B, d, page, fp8)
    if ragged:
        cu, lens = kv.cu_of(RAGGED_ROWS), RAGGED_LENS
        Knew, Vnew = mc.randn((cu[-1] + UNOWNED, mc.HKV, d), 801), mc.randn((cu[-1] + UNOWNED, mc.HKV, d), 802)
    else:
        cu, lens = None, APPEND_LENS
        Knew, Vnew = mc.randn((B, mc.HKV, APPEND_ROWS, d), 803), mc.randn((B, mc.HKV, APPEND_ROWS, d), 804)
    call = mc.append_call(base, Knew, Vnew, lens, cu)
    want = {"K": mc.appended(base, "K", Knew, lens, cu), "V": mc.appended(base, "V", Vnew, lens, cu)}
    assert not torch.equal(want["K"], ar.bits(base.K)), "the append changes the cache"

    def judge(v, what):
        for n in ("K", "V"):
            got = ar.bits(v[n]).cpu()
            assert (mc.kvc.same_bytes(got, want[n]) if fp8 else torch.equal(got, want[n])), f"{what}: {n} is not kv_append_check.append's"

    both_placements(call, judge, call.note)


# ---- e. one workspace, several calls ----------------------------------------------------------------------------------------------
def test_one_workspace_serves_several_calls():
    """as a serving engine uses its scratch: ONE arena workspace sized for the largest call; a decode (3 splits), an extend (2), a
    ragged windowed call (3) and a backward run on one stream with nothing cleared in between, each leaving in the workspace what the
    next one finds.  Every result is bit for bit its own fresh-workspace result"""
    d, H = 128, mc.HKV * mc.G
    c3, c4 = cache_of(3, d, 16, True), cache_of(4, d, None, False)
    cu = kv.cu_of(RAGGED_ROWS)
    Q, K, V, dO = backward_inputs(1, 4, 2, 100, 300, d, 901)
    calls = {
        "decode": mc.split_kv_call("decode", c3, mc.randn((3, H, 5, d), 911), LENS, True, 3, 0),
        "extend": mc.split_kv_call("extend", c3, mc.randn((3, H, 130, d), 912), LENS, True, 2, 0),
        "ragged": mc.split_kv_call("varlen", c4, mc.randn((cu[-1] + UNOWNED, H, d), 913), RAGGED_LENS, True, 3, 100, cu=cu),
        "backward": mc.backward_call(Q, K, V, dO, True, f32, f32),
    }
    assert all(c.ws_bytes > 0 for c in calls.values())
    fresh = {n: mc.run(c, None)[1] for n, c in calls.items()}
    specs = {"ws": mc.spec((max(c.ws_bytes for c in calls.values()),), mc.u8, writable=True)}
    data = {}
    for n, c in calls.items():
        specs.update({f"{n}.{k}": s for k, s in c.specs.items()})
        data.update({f"{n}.{k}": t for k, t in c.data.items()})
    for placement in mc.PLACEMENTS:
        arena, v = mc.place(mc.Call(specs, data, None, []), placement)
        for n, c in calls.items():
            mine = {k: v[f"{n}.{k}"] for k in c.specs}
            mine["ws"] = v["ws"]
            c.run(mine)                                        # no synchronisation, nothing cleared: the next call finds this one's scratch
        torch.cuda.synchronize()
        arena.check()
        for n, c in calls.items():
            for k in c.outs:
                got, want = v[f"{n}.{k}"], fresh[n][k]
                if n == "ragged":
                    got, want = (t[:cu[-1]] if k == "O" else t[:, :cu[-1]] for t in (got, want))
                assert mc.same(got, want), f"{n} [{placement}]: {k} differs from its fresh-workspace result"


# ---- f. refusal -------------------------------------------------------------------------------------------------------------------
def test_a_base_at_8_mod_16_is_refused_and_nothing_is_written():
    """Q, then O, then the workspace at 8 mod 16 through the Python fronts: FA_ERR_MISALIGNED before any launch"""
    d, S = 64, 96
    q = mc.randn((1, 2, S, d), 921)
    half = (8, 16)
    a = ar.Arena(DEV, 8 * ar.footprint((1, 2, S, d), f32))
    Q, K, V = (a.load(a.carve(q.shape, bf, name=n), q) for n in "QKV")
    Q8 = a.load(a.carve(q.shape, bf, half, name="Q8"), q)
    O, O8 = a.carve(q.shape, f32, name="O"), a.carve(q.shape, f32, half, name="O8")      # not writable: they must stay 0xFF
    for kw in (dict(Q=Q8, O=O), dict(Q=Q, O=O8)):
        with pytest.raises(fa.FlashAttentionError) as e:
            fa.flash_attention(kw["Q"], K, V, kw["O"], is_causal=True)
        assert e.value.code == FA_ERR_MISALIGNED
    lens = a.load(a.carve((1,), torch.int32, ar.SIDE, name="lens"), torch.tensor([S], dtype=torch.int32))
    need = fa.decode_workspace_size(1, 2, 5, d, 3)
    ws8 = a.carve((need,), torch.uint8, half, name="ws8")
    with pytest.raises(fa.FlashAttentionError) as e:
        fa.flash_attention_decode(Q[:, :, :5], K, V, lens, num_splits=3, O=O[:, :, :5], workspace=ws8)
    assert e.value.code == FA_ERR_MISALIGNED
    torch.cuda.synchronize()
    a.check()
