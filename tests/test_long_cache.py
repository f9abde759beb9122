"""GPU: the K/V-cache calls -- flash_attention_decode*, flash_attention_extend*, the ragged *_varlen calls and the _window forms, on
contiguous and paged, bf16 and e4m3fn caches -- on LONG caches: up to 2^20 keys per sequence, 2^24 at the capacity limit, pools past
2^32 bytes, thousands of pages and up to 64 splits, against the exact O(S d) closed forms of tests/long_cache_probe.py (CPU proof of the
instrument and of these cases' coverage: tests/test_long_cache_probe.py).  Every row of every sequence of every case is compared: O
BIT FOR BIT (V of the one key the row names, +0 where the mask, the window or the length hides it), the LSE within the derived
long_cache_probe.lse_bound; rows of a ragged O that no sequence owns keep a canary.  Data is built and compared on the device in
chunks.  The cases run from small caches to large ones, so that a defect shows where it is cheapest to read; a failure names sequence,
head, row, row block, and the target's key, tile, page and split.  What each case reached is in profiles/long_cache_gpu.log."""
import dataclasses
import time

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import long_cache_probe as cp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bf, f32 = torch.bfloat16, torch.float32
GIB = 2 ** 30
CASES = cp.gpu_cases()
BAD_SHAPE = -3                            # FA_ERR_BAD_SHAPE (include/flash_attention.h)


def cache_bytes(spec):
    rows = cp.layout(spec)[0] * spec.page if spec.page else len(spec.seqs) * spec.cap
    return 2 * rows * spec.Hkv * spec.d * spec.esz


def need(spec, extra=0.0):
    gib = cache_bytes(spec) / GIB * 1.25 + 2.0 + extra          # K and V, the builder's chunks, Q / O / slabs
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip(f"needs ~{gib:.1f} GiB of device memory")
    if spec.fp8 and cp.FP8 is None:
        pytest.skip("torch has no float8_e4m3fn")


_cache = {}


def cache_of(spec):
    """the caches of a spec, kept for the next case when it reads the same ones (the mask, and without a window the row counts, do not
    shape a cache)"""
    key = dataclasses.replace(spec, causal=True, kind="varlen" if spec.kind == "varlen" else "uniform",
                              seqs=tuple((s if spec.W or spec.kind == "varlen" else 1, L) for s, L in spec.seqs))
    if key not in _cache:
        _cache.clear()
        torch.cuda.empty_cache()
        _cache[key] = cp.build_cache(spec, DEV)
    return _cache[key]


def run(case, spec, cache, ns_asked, o_dtype=bf, W=None):
    """every round of the spec under the asked split count; prints the log line; -> (O, LSE) of the last round"""
    t0 = time.time()
    plan = cp.plan_of(spec, ns_asked, o_dtype, W)
    ns, rpb = plan["num_splits"], plan["rows_per_block"]
    rounds, missing = cp.plan_targets(spec, ns, rpb, cache["phys"])
    total = dict(rows=0, hidden=0, worst=0.0)
    for n, rnd in enumerate(rounds):
        q = cp.build_queries(spec, rnd, DEV)
        exp = cp.expected(spec, q, o_dtype, DEV)
        O = cp.canary_output(spec, o_dtype, DEV) if spec.kind == "varlen" else None
        O, lse = cp.call(spec, cache, q, ns_asked, o_dtype, W, O)
        torch.cuda.synchronize()
        got = cp.check(f"{case}, splits {ns_asked} -> {ns}, round {n}", spec, q, exp, O, lse, ns, rpb, cache)
        total = dict(rows=total["rows"] + got["rows"], hidden=total["hidden"] + got["hidden"], worst=max(total["worst"], got["worst"]))
    # (log labels only, as in cp.kernel_name: the names profiles/long_cache_gpu.log uses; the forms are the rows of csrc/split_forms.hip.h)
    combine = "" if ns == 1 else f" + {'extend_varlen_combine_kernel_of' if spec.kind == 'varlen' else 'decode_combine_kernel_of'}(d={spec.d})"
    keys = max(L for s, L in spec.seqs if s)
    print(f"{case}: {spec.form()}{f' W {W}' if W is not None else (f' W {spec.W}' if spec.W else '')}, {cp.kernel_name(spec, W)}{combine}, "
          f"{len(spec.seqs)} sequences, rows {sorted({s for s, _ in spec.seqs})}, longest {keys} keys (>= 2^17: {keys >= 2 ** 17}), capacity {spec.cap}, "
          f"H {spec.H} Hkv {spec.Hkv}, mask {spec.causal}, O {str(o_dtype)[6:]}, splits {ns_asked} -> {ns}, row blocks of {rpb}, {len(rounds)} rounds, "
          f"{len(missing)} forced places no row sees, {time.time() - t0:.2f} s, {total['rows']} rows compared bit for bit, "
          f"{total['hidden']} with a hidden target, worst LSE error / bound {total['worst']:.3f}")
    return O, lse


@pytest.mark.parametrize("case", sorted(CASES, key=lambda c: cache_bytes(CASES[c][0])))
def test_every_row_of_a_long_cache(case):
    spec, splits = CASES[case]
    need(spec)
    t0 = time.time()
    cache = cache_of(spec)
    torch.cuda.synchronize()
    print(f"\n{case}: caches of {cache_bytes(spec) / GIB:.2f} GiB built in {time.time() - t0:.2f} s")
    for n, ns in enumerate(splits):
        run(case, spec, cache, ns, f32 if n == 1 else bf)


def test_window_0_and_a_window_beyond_the_capacity_are_the_unwindowed_call():
    """5000 rows at length 2^20 - 3: flash_attention_extend, flash_attention_extend_window with W = 0 and with W = the capacity give the
    same bits -- and those are the closed form's (the first through run(); the window beyond the capacity through run() with W)"""
    spec = cp.Spec("extend", ((5000, 2 ** 20 - 3),), 2 ** 20, 128, seed=21)
    need(spec)
    cache = cache_of(spec)
    O0, L0 = run("unwindowed", spec, cache, 3)
    O1, L1 = run("window = capacity", spec, cache, 3, W=spec.cap)
    plan = cp.plan_of(spec, 3)
    q = cp.build_queries(spec, cp.plan_targets(spec, 3, plan["rows_per_block"])[0][-1], DEV)
    O2, L2 = fa.flash_attention_extend_window(q["Q"], cache["K"], cache["V"], kv_lens=cache["kv_lens"], window=0, scale=cp.fp.PREFILL_SCALE(0),
                                              is_causal=True, num_splits=3, return_lse=True, out_dtype=bf)
    torch.cuda.synchronize()
    for O, L in ((O1, L1), (O2, L2)):
        assert torch.equal(cp.lp._bits_of(O), cp.lp._bits_of(O0)) and torch.equal(cp.lp._bits_of(L), cp.lp._bits_of(L0))


def test_the_capacity_limit_is_2_pow_24_and_not_a_key_more():
    """Sk = 2^24 and max_pages * page = 2^24 are accepted (test_every_row_of_a_long_cache runs them); one key, one page more is
    FA_ERR_BAD_SHAPE, from the plan and from the call, before any launch"""
    if cp.FP8 is None:
        pytest.skip("torch has no float8_e4m3fn")
    spec = CASES["decode_fp8_at_the_capacity_limit_W0"][0]
    free, _ = torch.cuda.mem_get_info()
    if free < 4 * GIB:
        pytest.skip("needs ~4 GiB of device memory")
    assert cp.plan_of(spec)["num_splits"] >= 1
    with pytest.raises(fa.FlashAttentionError) as e:
        fa.decode_plan(1, 4, 1, 4, 2 ** 24 + 1, 64)
    assert e.value.code == BAD_SHAPE
    _cache.clear()
    K = torch.zeros((1, 1, 2 ** 24 + 16, 64), dtype=torch.uint8, device=DEV).view(cp.FP8)
    Q = torch.zeros((1, 4, 4, 64), dtype=bf, device=DEV)
    ones = torch.ones(1, dtype=f32, device=DEV)
    fa.flash_attention_decode(Q, K[:, :, :2 ** 24], K[:, :, :2 ** 24], kv_lens=torch.tensor([5], dtype=torch.int32, device=DEV), k_descale=ones, v_descale=ones)
    with pytest.raises(fa.FlashAttentionError) as e:
        fa.flash_attention_decode(Q, K[:, :, :2 ** 24 + 1], K[:, :, :2 ** 24 + 1], kv_lens=torch.tensor([5], dtype=torch.int32, device=DEV), k_descale=ones, v_descale=ones)
    assert e.value.code == BAD_SHAPE
    pool = torch.zeros((4, 1, 16, 64), dtype=bf, device=DEV)
    table = torch.zeros((1, 2 ** 20 + 1), dtype=torch.int32, device=DEV)
    lens = torch.tensor([5], dtype=torch.int32, device=DEV)
    fa.flash_attention_decode_paged(Q, pool, pool, table[:, :2 ** 20], kv_lens=lens)
    with pytest.raises(fa.FlashAttentionError) as e:
        fa.flash_attention_decode_paged(Q, pool, pool, table, kv_lens=lens)
    assert e.value.code == BAD_SHAPE
    torch.cuda.synchronize()


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_append_feeds_the_read(fp8):
    """a paged pool filled through kv_cache_append_paged_varlen in uneven chunks up to position 2^20 holds the bytes of the directly built
    pool -- asserted before any attention call -- and decode then reads it like the built one"""
    M = 2 ** 20
    spec = cp.Spec("decode", ((16, M), (16, 300032)), M, 128, fp8=fp8, page=128, seed=22)
    need(spec, extra=cache_bytes(spec) / GIB)
    t0 = time.time()
    built = cache_of(spec)
    K, V = cp._nan_like(built["K"].shape, spec, DEV), cp._nan_like(built["V"].shape, spec, DEV)
    chunks = [1, 4099, 65536, 17, 200000, 3, 131072, 300000, 64, 262144, 100000, M]
    pos, lens, steps = [0, 0], [L for _, L in spec.seqs], 0
    for c in chunks:
        sq = [min(c + 31 * b, lens[b] - pos[b]) for b in range(2)]
        if not any(sq):
            break
        Kn, Vn = torch.zeros((2, sum(sq), spec.Hkv, spec.d), dtype=bf, device=DEV)
        at = 0
        for b in range(2):
            for c0 in range(0, sq[b], cp.CHUNK):
                j = torch.arange(pos[b] + c0, pos[b] + min(c0 + cp.CHUNK, sq[b]), device=DEV)
                for kvh in range(spec.Hkv):
                    Kr, Vr = cp.key_rows(spec, j, kvh, b, lens[b], DEV)
                    Kn[at + c0:at + c0 + len(j), kvh] = (Kr * (cp.KD[kvh % 4] if fp8 else 1.0)).to(bf)
                    Vn[at + c0:at + c0 + len(j), kvh] = (Vr * (cp.VD[kvh % 4] if fp8 else 1.0)).to(bf)
            at += sq[b]
            pos[b] += sq[b]
        cu = torch.tensor([0, sq[0], sq[0] + sq[1]], dtype=torch.int32, device=DEV)
        fa.kv_cache_append_paged_varlen(Kn, Vn, K, V, built["table"], cu, torch.tensor(pos, dtype=torch.int32, device=DEV), built["kd"], built["vd"])
        steps += 1
    torch.cuda.synchronize()
    assert pos == lens
    for name, mine, ref in (("K", K, built["K"]), ("V", V, built["V"])):
        same = (cp.lp._bits_of(mine) == cp.lp._bits_of(ref)).all(-1).all(-1).all(-1)
        assert bool(same.all()), f"{name} pool: {int((~same).sum())} pages differ from the built pool, first pool page {int(torch.nonzero(~same)[0])}"
    print(f"\nappend {'fp8' if fp8 else 'bf16'}: {steps} ragged appends up to position {M}; both pools equal the built ones byte for byte, {time.time() - t0:.2f} s")
    run(f"decode on the appended pool ({'fp8' if fp8 else 'bf16'})", spec, dict(built, K=K, V=V), 3)


def test_the_row_count_side_2_pow_24_rows():
    """(run last: 13 GiB of tensors and slabs, more while they are built)  B H Sq = 2^24 rows of chunked prefill against small caches.  The
    combine kernel runs one 256-thread workgroup per row, and a launch of 2^32 threads is refused by the runtime (this test met
    hipErrorInvalidConfiguration, after the split kernel had run): FA_DECODE_MAX_WORKGROUPS now refuses two forced splits at 2^24 rows
    with FA_ERR_BAD_SHAPE; the library's choice there is one split, and the largest row count below runs under two.  Targets, caches and expectations are built on the device,
    vectorised over the batch (long_cache_probe's coding and closed forms; its per-row-block forced places are for the long caches)."""
    B, H, Hkv, Sq, cap, d, base = 2048, 8, 2, 1024, 1024, 64, 2 ** 24 - 2048
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * GIB:
        pytest.skip("needs ~24 GiB of device memory")
    _cache.clear()
    torch.cuda.empty_cache()
    t0 = time.time()
    G, nb = H // Hkv, 24
    g = torch.Generator(device=DEV).manual_seed(31)
    lens = (cap - 37 * (torch.arange(B, device=DEV) % 5)).to(torch.int32)
    j = torch.arange(cap, device=DEV)
    anc = cp.is_anchor(j)
    Krow = torch.zeros((cap, d), dtype=f32, device=DEV)
    Krow[:, :nb] = cp.lp.bits(base + j, nb).float()
    Krow[anc] = 0
    Krow[anc, nb] = 1
    K = Krow.to(bf).expand(B, Hkv, cap, d).contiguous()
    V = torch.empty((B, Hkv, cap, d), dtype=bf, device=DEV)
    Q = torch.empty((B, H, Sq, d), dtype=bf, device=DEV)
    expO = torch.empty((B, H, Sq, d), dtype=bf, device=DEV)
    expL = torch.empty((B, H, Sq), dtype=torch.float64, device=DEV)
    log2k = torch.empty((B, H, Sq), dtype=torch.float64, device=DEV)
    hidden = 0
    for b0 in range(0, B, 256):
        b = torch.arange(b0, b0 + 256, device=DEV)
        L = lens[b].long()
        for kvh in range(Hkv):
            v = cp.lp.v_rows((base + j)[None].expand(256, cap), (kvh + Hkv * b)[:, None, None], d).float()
            v[:, anc] = 0
            v = torch.where((j[None] >= L[:, None])[..., None], torch.full_like(v, float("nan")), v)
            V[b0:b0 + 256, kvh] = v.to(bf)
        lim = (L[:, None] - Sq + torch.arange(Sq, device=DEV)[None] + 1).clamp(min=1)[:, None].expand(256, H, Sq)
        r = torch.randint(0, 2 ** 31 - 1, (256, H, Sq), generator=g, device=DEV)
        n = torch.arange(H * Sq, device=DEV).view(H, Sq)[None]
        t = torch.where(n % 7 == 3, lim + r % cp.NEAR, torch.where(r % 2 == 0, (lim - 1 - (r >> 8) % cp.NEAR).clamp(min=0), (r >> 8) % lim)).clamp(1, cap - 1)
        t = torch.where(cp.is_anchor(t), t + 1, t)
        t = torch.where(t > cap - 1, torch.full_like(t, cap - 2), t)
        vis = t < lim
        hidden += int((~vis).sum())
        q = torch.zeros((256, H, Sq, d), dtype=f32, device=DEV)
        q[..., :nb] = cp.UNIT * cp.lp.bits(base + t, nb).float()
        q[..., nb] = cp.UNIT * nb - cp.E
        Q[b0:b0 + 256] = q.to(bf)
        salt = (torch.arange(H, device=DEV)[None] // G + Hkv * b[:, None])[..., None, None]
        o = torch.where(vis[..., None], cp.lp.v_rows(base + t, salt, d).float(), torch.zeros((), device=DEV)).to(bf)
        expO[b0:b0 + 256] = torch.where(o == 0, torch.full_like(o, cp.fp.ZERO_OUT), o)
        k = cp.anchors_below(lim).double()
        expL[b0:b0 + 256] = torch.where(vis, torch.full_like(k, cp.LN2 * cp.UNIT * nb), cp.LN2 * (cp.UNIT * nb - cp.E) + torch.log(k))
        log2k[b0:b0 + 256] = torch.where(vis, torch.zeros_like(k), torch.log2(k))
        del q, o, v
    assert B * H * Sq == 2 ** 24 == fa.FA_DECODE_MAX_WORKGROUPS
    kw = dict(scale=cp.fp.PREFILL_SCALE(0), is_causal=True, return_lse=True, out_dtype=bf)
    # two forced splits at 2^24 rows: FA_ERR_BAD_SHAPE from the plan and from the call, before any launch
    for refused in (lambda: fa.extend_plan(B, H, Hkv, Sq, cap, d, fa.FA_DTYPE_BF16, 2),
                    lambda: fa.flash_attention_extend(Q, K, V, kv_lens=lens, num_splits=2, **kw)):
        with pytest.raises(fa.FlashAttentionError) as e:
            refused()
        assert e.value.code == BAD_SHAPE
    # the library's choice at 2^24 rows is one split; two forced splits run on one sequence less: 2^24 - 8192 combine workgroups
    for what, nB, ns in (("2^24 rows, the library's choice", B, 0), ("2^24 - 8192 rows, two forced splits", B - 1, 2)):
        t1 = time.time()
        plan = fa.extend_plan(nB, H, Hkv, Sq, cap, d, fa.FA_DTYPE_BF16, ns)
        assert plan["num_splits"] == (ns or 1) and plan["combine_grid"] == (nB * H * Sq if ns else 0)
        O, lse = fa.flash_attention_extend(Q[:nB], K[:nB], V[:nB], kv_lens=lens[:nB], num_splits=ns, **kw)
        torch.cuda.synchronize()
        wrong = 0
        for b0 in range(0, nB, 256):
            bad = (cp.lp._bits_of(O[b0:b0 + 256]) != cp.lp._bits_of(expO[b0:min(b0 + 256, nB)])).any(-1)
            if bool(bad.any()) and not wrong:
                b, h, i = torch.nonzero(bad)[0].tolist()
                first = f"sequence {b0 + b} head {h} row {i}: {O[b0 + b, h, i, :6].float().tolist()} for {expO[b0 + b, h, i, :6].float().tolist()}"
            wrong += int(bad.sum())
        assert not wrong, f"{what}: {wrong} of {nB * H * Sq} rows differ from the closed form; first: {first}"
        ratio = (lse.double() - expL[:nB]).abs() / cp.lse_bound(expL[:nB], log2k[:nB])
        worst = float(torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf"))).max())
        print(f"\nrow-count side, {what}: extend contiguous bf16 d {d}, {cp.kernel_name(cp.Spec('extend', ((Sq, cap),), cap, d))}"
              f"{f' + decode_combine_kernel_of(d={d}) on ' + str(plan['combine_grid']) + ' workgroups' if ns else ''}, B {nB} H {H} Hkv {Hkv} Sq {Sq} "
              f"capacity {cap}, splits {ns} -> {plan['num_splits']}, {time.time() - t1:.2f} s (built in {t1 - t0:.2f} s), {nB * H * Sq} rows compared "
              f"bit for bit, {hidden} with a hidden target in the whole batch, worst LSE error / bound {worst:.3f}")
        assert worst <= 1.0
        del O, lse, ratio
