"""GPU tests of kv_cache_append and kv_cache_append_paged (flash_attention_kv_append, flash_attention_kv_append_paged): the write side
of the decode caches -- bf16 new rows copied into a bf16 cache or quantised to e4m3fn into an fp8 one, contiguous or paged, positions
and pages found on the device.

Everything here is a comparison of BITS with tests/kv_append_check.py, the contract written in torch on the CPU (held against a
brute-force round-to-nearest-even search in tests/test_kv_append_abi.py): no tolerance anywhere but in the end-to-end decode step,
whose O and LSE are held bit for bit against the same decode call on pools the CPU writer built, and against the float64 reference
of the decode tests at their stated 1e-3 + 1e-3 |ref| / 2e-4 + 2e-6 |ref|.  NaN bytes are compared by class, (b & 0x7F) == 0x7F.

The caches are handled as integer tensors (uint8: e4m3fn bytes, int16: bf16 patterns), pre-filled with a sentinel, compared WHOLE --
so every byte that must not be written is checked with the ones that must -- and viewed as float8_e4m3fn / bfloat16 at the call."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import kv_append_check as kc  # noqa: E402
from kv_append_check import SENT, as_cache, descales, new_rows, same, sentinel  # noqa: E402
from kv_cache_check import DEV, assert_close, dequantise, gather, i32 as lens_tensor, reference  # noqa: E402

pytestmark = pytest.mark.gpu
bf, i16, u8, i32 = torch.bfloat16, torch.int16, torch.uint8, torch.int32
HKV = 2
def dev(t):
    return None if t is None else t.to(DEV)


# ---- 1. every bf16 value ----
def test_every_bf16_value():
    Hkv, Sq, d = 4, 512, 128
    pat = kc.all_bf16_patterns().reshape(Sq, d)
    Kn = pat[None, None].expand(1, Hkv, Sq, d).contiguous()
    Vn = pat.flip(0, 1)[None, None].expand(1, Hkv, Sq, d).contiguous()
    kd, vd = torch.tensor([1.0, 0.25, 0.0123, 3.7]), torch.tensor([3.7, 0.0123, 1.0, 0.25])
    lens = [Sq]
    for fp8 in (True, False):
        Kc, Vc = sentinel((1, Hkv, Sq, d), fp8, DEV), sentinel((1, Hkv, Sq, d), fp8, DEV)
        ds = dict(k_descale=dev(kd), v_descale=dev(vd)) if fp8 else {}
        fa.kv_cache_append(dev(Kn), dev(Vn), as_cache(Kc), as_cache(Vc), lens_tensor(lens), **ds)
        torch.cuda.synchronize()
        wantK = kc.append(Kn, sentinel((1, Hkv, Sq, d), fp8), lens, kd)
        wantV = kc.append(Vn, sentinel((1, Hkv, Sq, d), fp8), lens, vd)
        if fp8:
            for h in range(Hkv):      # say which patterns, if any
                bad = (Kc[0, h].cpu() != wantK[0, h]) & ((wantK[0, h] & 0x7F) != 0x7F)
                assert not bad.any(), (h, float(kd[h]), [hex(int(v)) for v in pat.view(i16)[bad][:8].int() & 0xFFFF],
                                       [hex(int(v)) for v in Kc[0, h].cpu()[bad][:8]], [hex(int(v)) for v in wantK[0, h][bad][:8]])
        else:
            assert torch.equal(Kc.cpu().reshape(Hkv, -1).int() & 0xFFFF, torch.arange(65536, dtype=i32).expand(Hkv, -1))   # a bit copy
        assert same(Kc, wantK) and same(Vc, wantV), fp8
    # a NULL descale is 1.0
    Kc, Vc = sentinel((1, Hkv, Sq, d), True, DEV), sentinel((1, Hkv, Sq, d), True, DEV)
    fa.kv_cache_append(dev(Kn), dev(Vn), as_cache(Kc), as_cache(Vc), lens_tensor(lens), v_descale=dev(vd))
    torch.cuda.synchronize()
    assert same(Kc, kc.append(Kn, sentinel((1, Hkv, Sq, d), True), lens, None)) and same(Vc, kc.append(Vn, sentinel((1, Hkv, Sq, d), True), lens, vd))


# ---- 2. positions ----
def position_lengths(Sq, cap):
    return [-3, 0, 1, 2, Sq - 1, Sq, Sq + 1, 127, 128, 129, cap - 1, cap, cap + 7]


@pytest.mark.parametrize("fp8", [True, False])
@pytest.mark.parametrize("d,cap", [(64, 384), (128, 320)])
def test_positions(d, cap, fp8):
    for Sq in (1, 3, 16, 40):
        lens = position_lengths(Sq, cap)
        B = len(lens)
        Kn, Vn = new_rows((B, HKV, Sq, d), 10 + Sq + d), new_rows((B, HKV, Sq, d), 20 + Sq + d)
        kd, vd = descales(30 + Sq, fp8)
        ds = dict(k_descale=dev(kd), v_descale=dev(vd)) if fp8 else {}
        for L in (lens, None):
            Kc, Vc = sentinel((B, HKV, cap, d), fp8, DEV), sentinel((B, HKV, cap, d), fp8, DEV)
            fa.kv_cache_append(dev(Kn), dev(Vn), as_cache(Kc), as_cache(Vc), lens_tensor(L), **ds)
            torch.cuda.synchronize()
            wantK, wantV = kc.append(Kn, sentinel((B, HKV, cap, d), fp8), L, kd), kc.append(Vn, sentinel((B, HKV, cap, d), fp8), L, vd)
            assert same(Kc, wantK) and same(Vc, wantV), (Sq, L)
            # (the reference wrote what the header says: nothing for L <= 0, min(L, Sq) rows ending at min(L, cap) otherwise)
            written = (wantK != SENT[wantK.dtype]).any(-1).any(1).sum(-1).tolist()
            assert written == [min(max(min(x, cap), 0), Sq) for x in (L or [cap] * B)], (Sq, L)


# ---- 3. paged ----
def paged_case(page, Sq, d, fp8, spare=5):
    n = max(3, 320 // page)
    cap = n * page
    lens = sorted({max(1, min(L, cap)) for L in (1, Sq, page - 1, page, page + 1, 127, 128, 129, cap - 3, cap)}) + [0]
    B = len(lens)
    P = B * n + spare
    g = torch.Generator().manual_seed(400 + page + Sq)
    table = torch.randperm(P, generator=g)[:B * n].reshape(B, n).to(i32)
    Kn, Vn = new_rows((B, HKV, Sq, d), 40 + Sq + page), new_rows((B, HKV, Sq, d), 50 + Sq + page)
    kd, vd = descales(60 + page, fp8)
    return n, cap, lens, B, P, table, Kn, Vn, kd, vd


def run_paged(Kn, Vn, P, page, d, fp8, table_dev, lens, kd, vd):
    Kp, Vp = sentinel((P, HKV, page, d), fp8, DEV), sentinel((P, HKV, page, d), fp8, DEV)
    ds = dict(k_descale=dev(kd), v_descale=dev(vd)) if fp8 else {}
    fa.kv_cache_append_paged(dev(Kn), dev(Vn), as_cache(Kp), as_cache(Vp), table_dev, lens_tensor(lens), **ds)
    torch.cuda.synchronize()
    return Kp, Vp


@pytest.mark.parametrize("fp8", [True, False])
@pytest.mark.parametrize("page", [16, 64, 128])
def test_paged(page, fp8):
    d = 64 if page == 64 else 128
    for Sq in (1, 7, 40):
        n, cap, lens, B, P, table, Kn, Vn, kd, vd = paged_case(page, Sq, d, fp8)
        Kp, Vp = run_paged(Kn, Vn, P, page, d, fp8, dev(table), lens, kd, vd)
        empty = sentinel((P, HKV, page, d), fp8)
        wantK, wantV = kc.append(Kn, empty, lens, kd, table), kc.append(Vn, empty, lens, vd, table)
        assert same(Kp, wantK) and same(Vp, wantV), Sq                  # (spare pages and unwritten rows: the sentinel, in there)
        # the contiguous call on the same rows gives the gathered pools, bit for bit
        Kc, Vc = sentinel((B, HKV, cap, d), fp8, DEV), sentinel((B, HKV, cap, d), fp8, DEV)
        ds = dict(k_descale=dev(kd), v_descale=dev(vd)) if fp8 else {}
        fa.kv_cache_append(dev(Kn), dev(Vn), as_cache(Kc), as_cache(Vc), lens_tensor(lens), **ds)
        torch.cuda.synchronize()
        assert torch.equal(gather(Kp, dev(table)), Kc) and torch.equal(gather(Vp, dev(table)), Vc), Sq
        # entries of pages that receive no row are not read: any int32 there, the same pools
        receives = torch.zeros(B, n, dtype=torch.bool)
        for b, L in enumerate(lens):
            for _, p in kc.positions(L, Sq, cap):
                receives[b, p // page] = True
        assert int((~receives).sum()) > 0
        for junk in (-1, 2 ** 31 - 1, P + 5):
            t2 = torch.where(receives, table, torch.full_like(table, junk))
            K2, V2 = run_paged(Kn, Vn, P, page, d, fp8, dev(t2), lens, kd, vd)
            assert torch.equal(K2, Kp) and torch.equal(V2, Vp), (Sq, junk)
        # entries AT written positions outside [0, P): those rows are skipped (not clamped into another page), the rest as before
        hit = receives.nonzero()
        t3 = table.clone()
        for k, (b, j) in enumerate(hit[::2].tolist()):
            t3[b, j] = (-1, P, 2 ** 31 - 1, -2 ** 31, P + 5)[k % 5]
        K3, V3 = run_paged(Kn, Vn, P, page, d, fp8, dev(t3), lens, kd, vd)
        want3 = kc.append(Kn, empty, lens, kd, t3)
        skipped = torch.zeros(P, dtype=torch.bool)
        skipped[table[t3 != table].long()] = True
        assert same(K3, want3) and same(V3, kc.append(Vn, empty, lens, vd, t3)), Sq
        assert torch.equal(K3.cpu()[~skipped], Kp.cpu()[~skipped]) and bool((K3.cpu()[skipped] == SENT[K3.dtype]).all()), Sq
        # a row slice of a wider table
        wide = torch.full((B, n + 5), -7, dtype=i32)
        wide[:, 3:3 + n] = table
        K4, V4 = run_paged(Kn, Vn, P, page, d, fp8, dev(wide)[:, 3:3 + n], lens, kd, vd)
        assert torch.equal(K4, Kp) and torch.equal(V4, Vp), Sq


# ---- 4. layouts ----
@pytest.mark.parametrize("fp8", [True, False])
@pytest.mark.parametrize("d", [64, 128])
def test_layouts(d, fp8):
    B, Sq, H, cap, page = 3, 5, 6, 320, 16
    lens = [cap, 131, 4]
    kd, vd = descales(70 + d, fp8)
    ds = dict(k_descale=dev(kd), v_descale=dev(vd)) if fp8 else {}
    # the K and V slices of one fused [B, Sq, (H + 2 Hkv) d] projection
    fused = new_rows((B, Sq, (H + 2 * HKV) * d), 71 + d)
    heads = fused.view(B, Sq, H + 2 * HKV, d)
    Kn, Vn = heads[:, :, H:H + HKV].transpose(1, 2), heads[:, :, H + HKV:].transpose(1, 2)
    fd = dev(fused).view(B, Sq, H + 2 * HKV, d)
    Knd, Vnd = fd[:, :, H:H + HKV].transpose(1, 2), fd[:, :, H + HKV:].transpose(1, 2)
    assert not Knd.is_contiguous() and Knd.shape == (B, HKV, Sq, d)
    wantK, wantV = kc.append(Kn, sentinel((B, HKV, cap, d), fp8), lens, kd), kc.append(Vn, sentinel((B, HKV, cap, d), fp8), lens, vd)
    # ... into a [B, S, Hkv, d] cache
    Kc, Vc = sentinel((B, cap, HKV, d), fp8, DEV), sentinel((B, cap, HKV, d), fp8, DEV)
    fa.kv_cache_append(Knd, Vnd, as_cache(Kc).transpose(1, 2), as_cache(Vc).transpose(1, 2), lens_tensor(lens), **ds)
    torch.cuda.synchronize()
    assert same(Kc.transpose(1, 2), wantK) and same(Vc.transpose(1, 2), wantV)
    # ... into a [P, page, Hkv, d] pool
    n = cap // page
    P = B * n + 3
    table = torch.randperm(P, generator=torch.Generator().manual_seed(72))[:B * n].reshape(B, n).to(i32)
    Kp, Vp = sentinel((P, page, HKV, d), fp8, DEV), sentinel((P, page, HKV, d), fp8, DEV)
    fa.kv_cache_append_paged(Knd, Vnd, as_cache(Kp).transpose(1, 2), as_cache(Vp).transpose(1, 2), dev(table), lens_tensor(lens), **ds)
    torch.cuda.synchronize()
    empty = sentinel((P, HKV, page, d), fp8)
    assert same(Kp.transpose(1, 2), kc.append(Kn, empty, lens, kd, table)) and same(Vp.transpose(1, 2), kc.append(Vn, empty, lens, vd, table))
    # row strides d + 16 (K) and d + 32 (V), new rows and caches: the padding between rows keeps what it held
    for padK, padV in ((16, 32),):
        rawKn, rawVn = new_rows((B, HKV, Sq, d + padK), 73 + d), new_rows((B, HKV, Sq, d + padV), 74 + d)
        rawK, rawV = sentinel((B, HKV, cap, d + padK), fp8, DEV), sentinel((B, HKV, cap, d + padV), fp8, DEV)
        fa.kv_cache_append(dev(rawKn)[..., :d], dev(rawVn)[..., :d], as_cache(rawK)[..., :d], as_cache(rawV)[..., :d], lens_tensor(lens), **ds)
        torch.cuda.synchronize()
        for raw, rawn, pad, dsc in ((rawK, rawKn, padK, kd), (rawV, rawVn, padV, vd)):
            want = sentinel((B, HKV, cap, d + pad), fp8)
            want[..., :d] = kc.append(rawn[..., :d], sentinel((B, HKV, cap, d), fp8), lens, dsc)
            assert same(raw, want), pad


# ---- 5. a pool above 2^32 bytes ----
def test_page_bases_are_64_bit():
    page, d, Sq = 128, 128, 3
    per_page = HKV * page * d                       # bytes of one fp8 page
    P = (1 << 32) // per_page + 8
    Kp, Vp = torch.empty((P, HKV, page, d), dtype=u8, device=DEV), torch.empty((P, HKV, page, d), dtype=u8, device=DEV)
    assert Kp.numel() > 1 << 32
    hi = P - 3
    alias = hi - (1 << 32) // per_page              # where a 32-bit byte offset of page `hi` would land
    assert 0 <= alias < P and hi * per_page >= 1 << 32
    for pool in (Kp, Vp):
        pool[hi] = SENT[u8]
        pool[alias] = SENT[u8]
    table = torch.tensor([[alias + 1, hi, alias + 2]], dtype=i32)     # positions 128 .. 255 live in page `hi`
    lens = [page + 70]
    Kn, Vn = new_rows((1, HKV, Sq, d), 80), new_rows((1, HKV, Sq, d), 81)
    kd, vd = descales(82, True)
    fa.kv_cache_append_paged(dev(Kn), dev(Vn), as_cache(Kp), as_cache(Vp), dev(table), lens_tensor(lens), k_descale=dev(kd), v_descale=dev(vd))
    torch.cuda.synchronize()
    for pool, new, ds in ((Kp, Kn, kd), (Vp, Vn, vd)):
        want = sentinel((1, HKV, page, d), True)
        want[0, :, 70 - Sq:70] = kc.encode(new, ds, True)[0]
        assert kc.same_bytes(pool[hi][None], want)
        assert bool((pool[alias] == SENT[u8]).all())


# ---- 6. a decode step end to end, one graph ----
@pytest.mark.parametrize("fp8,Sq,d,window", [(True, 1, 128, 0), (True, 4, 64, 0), (False, 1, 64, 0), (False, 4, 128, 0), (True, 4, 128, 16)])
def test_decode_step_in_one_graph(fp8, Sq, d, window):
    B, G, page, n, steps = 2, 2, 16, 20, 6
    H, cap = G * HKV, n * page
    start = [125, 13]
    P = B * n + 5
    table = torch.randperm(P, generator=torch.Generator().manual_seed(90 + Sq))[:B * n].reshape(B, n).to(i32)
    kd, vd = (torch.tensor([0.02, 0.031]), torch.tensor([0.017, 0.025])) if fp8 else (None, None)
    rows = lambda shape, seed: torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(bf)
    # the history: the CPU writer fills the pools up to the starting lengths
    refK, refV = sentinel((P, HKV, page, d), fp8), sentinel((P, HKV, page, d), fp8)
    for b, L in enumerate(start):
        one = [L if x == b else 0 for x in range(B)]
        refK = kc.append(rows((B, HKV, L, d), 91 + b), refK, one, kd, table)
        refV = kc.append(rows((B, HKV, L, d), 93 + b), refV, one, vd, table)
    Kp, Vp, td = dev(refK), dev(refV), dev(table)
    lens = torch.tensor(start, dtype=i32, device=DEV)
    Kn_s, Vn_s = torch.zeros((B, HKV, Sq, d), dtype=bf, device=DEV), torch.zeros((B, HKV, Sq, d), dtype=bf, device=DEV)
    Q_s = torch.zeros((B, H, Sq, d), dtype=bf, device=DEV)
    O_s = torch.zeros((B, H, Sq, d), dtype=torch.float32, device=DEV)
    ns = 2
    ws = torch.empty(fa.decode_workspace_size(B, H, Sq, d, ns), dtype=u8, device=DEV)
    ds = dict(k_descale=dev(kd), v_descale=dev(vd)) if fp8 else {}
    dkw = dict(is_causal=True, num_splits=ns, window=window or None, return_lse=True, **ds)

    def step():
        lens.add_(Sq)
        fa.kv_cache_append_paged(Kn_s, Vn_s, as_cache(Kp), as_cache(Vp), td, lens, **ds)
        return fa.flash_attention_decode_paged(Q_s, as_cache(Kp), as_cache(Vp), td, lens, O=O_s, workspace=ws, **dkw)

    step()                                    # (first calls outside the capture; then the state as it was)
    torch.cuda.synchronize()
    lens.copy_(torch.tensor(start, dtype=i32))
    Kp.copy_(refK)
    Vp.copy_(refV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, lse_s = step()
    lens.copy_(torch.tensor(start, dtype=i32))      # (capture runs nothing, but say so)
    now = list(start)
    for t in range(steps):
        Kn, Vn, Q = rows((B, HKV, Sq, d), 100 + t), rows((B, HKV, Sq, d), 200 + t), rows((B, H, Sq, d), 300 + t)
        Kn_s.copy_(Kn)
        Vn_s.copy_(Vn)
        Q_s.copy_(Q)
        graph.replay()
        torch.cuda.synchronize()
        now = [L + Sq for L in now]
        assert lens.tolist() == now
        refK, refV = kc.append(Kn, refK, now, kd, table), kc.append(Vn, refV, now, vd, table)
        assert same(Kp, refK) and same(Vp, refV), t
        O, lse = O_s.clone(), lse_s.clone()
        # the same decode call on the pools the CPU writer built: the same bits
        O2, lse2 = fa.flash_attention_decode_paged(dev(Q), as_cache(dev(refK)), as_cache(dev(refV)), td, lens, out_dtype=torch.float32, **dkw)
        torch.cuda.synchronize()
        assert torch.equal(O, O2) and torch.equal(lse, lse2), t
        # ... and the float64 reference on the values the cache holds
        Kg, Vg = gather(refK, table), gather(refV, table)
        Kf, Vf = (dequantise(Kg, kd), dequantise(Vg, vd)) if fp8 else (Kg.view(bf), Vg.view(bf))
        refO, refL = reference(Q, Kf, Vf, now, True, window)
        assert_close(O, lse, refO, refL, f"decode step {t} fp8 {fp8} Sq {Sq} d {d} window {window} lengths {now}")
    assert now[0] > 128 >= start[0] and now[1] > 16 >= start[1]          # the steps crossed the tile and a page boundary


# ---- 7. determinism and streams ----
@pytest.mark.parametrize("fp8", [True, False])
def test_the_same_call_gives_the_same_bytes_and_a_side_stream_orders_it(fp8):
    B, Sq, d, cap = 4, 40, 128, 320
    lens = [cap, 200, 41, 7]
    Kn, Vn = new_rows((B, HKV, Sq, d), 110), new_rows((B, HKV, Sq, d), 111)
    kd, vd = descales(112, fp8)
    ds = dict(k_descale=dev(kd), v_descale=dev(vd)) if fp8 else {}
    wantK, wantV = kc.append(Kn, sentinel((B, HKV, cap, d), fp8), lens, kd), kc.append(Vn, sentinel((B, HKV, cap, d), fp8), lens, vd)
    got = []
    for _ in range(2):
        Kc, Vc = sentinel((B, HKV, cap, d), fp8, DEV), sentinel((B, HKV, cap, d), fp8, DEV)
        fa.kv_cache_append(dev(Kn), dev(Vn), as_cache(Kc), as_cache(Vc), lens_tensor(lens), **ds)
        torch.cuda.synchronize()
        got.append((Kc, Vc))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and same(got[0][0], wantK) and same(got[0][1], wantV)
    # a side stream: the new rows are produced on it just before the call, and the result is read after it alone is waited for
    side = torch.cuda.Stream()
    Knd, Vnd, ld = dev(Kn), dev(Vn), lens_tensor(lens)
    stage_k, stage_v = torch.zeros_like(Knd), torch.zeros_like(Vnd)
    Kc, Vc = sentinel((B, HKV, cap, d), fp8, DEV), sentinel((B, HKV, cap, d), fp8, DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        stage_k.copy_(Knd)
        stage_v.copy_(Vnd)
    fa.kv_cache_append(stage_k, stage_v, as_cache(Kc), as_cache(Vc), ld, stream=side, **ds)
    side.synchronize()
    assert same(Kc, wantK) and same(Vc, wantV)
