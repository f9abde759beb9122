#!/usr/bin/env python3
"""Time flash_attention_decode (split-KV decode): one JSON line per shape.

  python3 tools/bench_decode.py [--steps N] [--warmup W] [--repeats R] [--shape NAME ...] [--splits 1,2,4,...] [--no-cross]
                                [--paged 16,128,256] [--kv fp8] [--window 128,4096] [--append] [--extend | --varlen] [--sinks] [--rope]
                                [--tree 8,16,64] [--mla]

Shapes (bf16 in / bf16 out, d = 128 unless named, Sq new rows against a cache of capacity Sk):
  single_32k B1 H32 Hkv8 Sq1 Sk32768      single_128k B1 H32 Hkv8 Sq1 Sk131072    batch8_8k B8 H32 Hkv8 Sq1 Sk8192
  batch64_4k B64 H64 Hkv8 Sq1 Sk4096      mha_16k B4 H32 Hkv32 Sq1 Sk16384        spec4_32k B8 H32 Hkv8 Sq4 Sk32768
  d64_16k B8 H32 Hkv8 Sq1 Sk16384 d64     ragged B16 H32 Hkv8 Sq1 capacity 32768, lengths spread 1 k ... 32 k
Each line:
  ms          one flash_attention_decode call (its launches and the Python binding; O and the workspace given), hipEvents around
              --steps calls after --warmup calls; the median of --repeats such windows, ms_min / ms_max their spread.  The device
              is primed first with >= 1 s of calls
  kv_TBps     unique K/V bytes actually visible (sum over the batch of kv_lens x Hkv x d x 2 tensors x 2 bytes) / ms
  kv_MB       those bytes: above the 256 MiB Infinity Cache the figure shows HBM, below it the cache
  splits, grid  what the library planned (or --splits forced)
  cross_ms    the same problem through flash_attention() (no mask, uniform length = capacity, grouped-query tensors): what a caller
              had to issue before this path existed; speedup = cross_ms / ms
--paged a,b,c   page sizes: per shape, the same K/V data scattered into pools of such pages behind a SHUFFLED block table, through
              flash_attention_decode_paged (same lengths, O, workspace and plan as `ms`): paged_ms[page] with its min / max and
              paged_ratio[page] = paged_ms / ms (profiles/decode_paged_bench.log).
--kv fp8        per shape, the same call against the fp8 cache of that shape: the bf16 K/V quantised to float8_e4m3fn per K/V head
              (descale = amax / 448), same Q, lengths, O, workspace and plan as `ms` and timed the same way in the same run: fp8_ms
              with its min / max, fp8_ratio = fp8_ms / ms, and fp8_kv_tbps from the bytes actually read (one per element: kv_MB / 2).
              With --paged, paged_fp8_ms[page] as well: the fp8 pools behind the same shuffled table
              (profiles/decode_fp8_bench.log).
--window a,b,c  sliding windows: per shape and window W, the same call with window=W (same Q, cache, lengths and O; the plan and the
              workspace are the window's): window_ms[W] with its min / max, window_splits[W], and window_kv_tbps[W] from the bytes of
              the keys a windowed sequence can see (sum over the batch of min(kv_lens, W + Sq - 1) keys; window_kv_MB[W]).  With
              --kv fp8 window_fp8_ms[W] / window_fp8_kv_tbps[W] as well, with --paged window_paged_ms[page][W] (and
              window_paged_fp8_ms[page][W]) (profiles/decode_window_bench.log).
--append        the write side (kv_cache_append, kv_cache_append_paged): per shape and cache form -- "bf16", with --kv fp8 "fp8", with
              --paged "paged<page>" (and "paged<page>_fp8"), behind a shuffled block table -- timed like `ms` in the same run:
              append_ms[form]       one call that appends the shape's own Sq new rows per sequence at the shape's lengths (K and V)
              torch_append_ms[form] the same result built with torch ops on the same data: positions (and pages) from kv_lens and the
                                    table on the device, kv_cache_check.quantise's expression with the given descales, one indexed
                                    write per tensor; append_matches_torch[form]: the two caches hold the same bytes
              fill_ms[form], fill_tbps[form]  one call with Sq = 4096 and kv_lens = None (the cache's last 4096 rows: a fill after a
                                    prefill); bytes read + written = B Hkv 4096 d x 2 tensors x (2 + bytes per cache element)
              each with _min / _max over the windows (profiles/kv_append_bench.log).
--rope          the append with the rotary embedding fused in (rope_cache_append, rope_cache_append_paged) beside the routes without it: a
              mode of its own over the --append shapes, one line per shape, every figure per cache form ("bf16", with --kv fp8 "fp8",
              with --paged "paged<page>" and "paged<page>_fp8"); full rotary (rot_dim = d), half-split pairs, the shape's lengths:
              rope_append_ms[form]  one fused call: Q and K rotated, K and V into the cache, Qout written
              unfused_ms[form]      what a caller does today: torch ops that take the positions from kv_lens on the device, gather
                                    cos / sin, rotate Q and K in fp32 and round them to bf16, then kv_cache_append* of the rotated K
              append_ms[form]       the plain kv_cache_append* of the same rows: the floor (no Q traffic, no rotation)
              the three ALTERNATED, --repeats windows of --steps calls each; _min / _max their spread
              rope_matches_unfused[form]  the two routes agree as far as their arithmetic lets them: torch rounds x1 c and x2 s each
                                    to fp32 before the subtraction, the fused expression one of them, so before the rounding to bf16
                                    the two differ by at most 2^-23 (|x1| + |x2|).  Qout and a bf16 K cache: |a - b| <= one bf16 ulp
                                    of the larger, 2^-7 max(|a|, |b|), plus 2^-21 of the largest |x|; an fp8 K cache: codes one
                                    apart at the most; the V cache: the same bytes
              rope_fill_ms, unfused_fill_ms, fill_ms, q_copy_fill_ms[form]  (Sk >= 4096) the same three with Sq = 4096 and
                                    kv_lens = None, and a plain bf16 copy of that Q: the fused fill is expected near fill_ms +
                                    q_copy_fill_ms (profiles/rope_append_gpu.log).
--splits a,b,c  the forced-split sweep: one line per (shape, split count) with ms only (profiles/decode_split_sweep.log).
--extend        flash_attention_extend / flash_attention_extend_paged (chunked prefill against the decode caches) instead of decode:
              one line per shape and cache form -- "bf16", with --kv fp8 "fp8", with --paged "paged<page>" (and "paged<page>_fp8") --
              over its own shapes (H32 Hkv8, d = 128 unless named; a chunk of Sq new rows behind a cached prefix, kv_lens = prefix + Sq):
                chunk512_8k B1 Sq512 prefix 8192    chunk512_32k B1 Sq512 prefix 32768    chunk2048_0 B1 Sq2048 no prefix
                chunk64_32k B1 Sq64 prefix 32768    batch8_ragged B8 Sq512 prefixes spread 1 k ... 32 k    d64_chunk512_8k d64
              extend_ms         one call (O and the workspace given), timed like `ms`; splits, row_blocks, rows_per_block, grid: its plan
              sliced_decode_ms  what the decode call can do for the same result: flash_attention_decode* over 16-row slices of Q,
                                slice j with the lengths kv_lens - Sq + 16 (j + 1) (per-slice length tensors built beforehand);
                                extend_vs_sliced_max_abs: the largest difference of the two results
              prefill_pair_ms   ("bf16" only) what the prefill call can do: flash_attention (grouped-query) not causal over the prefix
                                view plus causal over the chunk's own keys, both with their LSE, merged with torch ops in fp32 -- per
                                sequence where the prefixes differ; pair_vs_extend_max_abs likewise
              gather_ms, dequantise_ms  (paged / fp8 forms) the torch gather into a contiguous cache and the dequantisation to bf16
                                that the prefill route would need first, each timed on its own
              each with _min / _max over the windows (profiles/extend_bench.log).  With --splits: the forced
              sweep of flash_attention_extend on the bf16 cache, one line per (shape, split count).
--varlen        flash_attention_extend_varlen / flash_attention_extend_paged_varlen (ragged chunked prefill: a per-sequence row count,
              Q / O packed by token) on mixed batches: one line per shape and cache form ("bf16", --kv fp8, --paged as for --extend).
              Shapes (H32 Hkv8, causal, d = 128 and, named d64_..., d = 64; kv_lens = prefix + rows):
                decode63_chunk512  63 decoding sequences (1 row) on 8 k ... 32 k, plus one 512-row chunk on 8 k
                chunks8_64_1024    8 chunks of 64, 128, 192, 256, 384, 512, 768, 1024 rows on 1 k ... 32 k
                uniform8x512_8k    8 x 512 rows on 8 k           decode64_16k  64 x 1 row on 16 k
              varlen_ms         one ragged call (O and the workspace given), timed like `ms`; splits, row_blocks_bound (the plan's NB),
                                row_blocks_real (what the lookup finds), rows_per_block, grid: its plan
              grouped_ms        what a caller does today: one flash_attention_decode* for the 1-row sequences plus one
                                flash_attention_extend* per distinct chunk length (grouped_calls of them), on PRE-GROUPED tensors --
                                the regrouping copies are not charged; varlen_vs_grouped_max_abs: the largest difference
              regroup_ms        those copies on their own: Q from token-major into [Bg, H, rows, d] per group, O back
              extend_ms / ms    (a uniform batch: one group) grouped_ms under the name of the call it is -- the same problem through
                                flash_attention_extend (the cost of being ragged) or, 1-row sequences only, through
                                flash_attention_decode (the cost of row blocks of 32 / 64 rows on decode rows)
              append_varlen_ms  one kv_cache_append*_varlen call for the batch's new rows; append_ms: today's, one kv_cache_append*
                                call per group on pre-grouped new rows
              each with _min / _max over the windows (profiles/extend_varlen_bench.log).  With --splits: the
              forced sweep of the ragged call on the bf16 cache, one line per (shape, split count).
--window with --extend / --varlen   the windowed calls (flash_attention_extend*_window, flash_attention_extend*_varlen_window)
              beside the un-windowed call of the same shape in the same run: per cache form, extend_window_ms[W] / varlen_window_ms[W]
              with their _min / _max and window_splits[W] (the window's plan) next to extend_ms / varlen_ms; the comparison routes
              (sliced decode, prefill pair, grouped calls, appends) are not timed.  --extend --window adds two shapes, B1 behind a
              32 k prefix: chunk1024_32k (Sq a multiple of rows_per_block) and chunk1000_32k (it is not: the row blocks that straddle
              two heads walk the whole chunk's span).  With --splits: the forced sweep, one line per (shape, split count) with
              extend_ms / varlen_ms and the windowed times at that count (profiles/extend_window_bench.log).
--sinks         attention sinks (``sinks=``: the flash_attention_sink_* entry points) beside the same call without them: a mode of its own
              over the shapes of decode, --extend or --varlen.  One line per shape and cache form ("bf16", with --kv fp8 "fp8", with --paged
              "paged<page>" and "paged<page>_fp8"), every figure per window (0 = none, then every --window value): the two calls share Q, the cache,
              the lengths, O, the plan and the workspace, and are timed ALTERNATED -- --repeats times (a window of --steps calls without
              sinks, then one with) -- after the usual priming:
              ms       the call without sinks: [median, min, max] of its windows -- min .. max is the noise of this run
              sink_ms  the call with sinks (a [H] vector of logits around the row's LSE), likewise
              sink_ratio = sink_ms / ms (medians); splits: the plan both calls run under (profiles/sink_bench.log).
--tree N[,N...] tree-masked verification (flash_attention_tree*) beside its causal twin: a mode of its own over the decode shapes with N draft
              nodes per sequence in place of Sq.  One line per shape and cache form (as under --sinks), every figure per N: the twin --
              flash_attention_sink_decode* up to 16 nodes, flash_attention_sink_extend* above, is_causal -- and the tree call share Q, the
              cache, the lengths, the sinks and the plan (the window: the first --window value, else none), both allocate O and the
              workspace themselves, and they are timed ALTERNATED, --repeats windows of --steps calls each, after the usual priming:
              causal_ms  the twin: [median, min, max] of its windows -- min .. max is the noise of this run
              tree_ms    the tree call under a heap-shaped binary-tree mask, likewise
              tree_ratio = tree_ms / causal_ms (medians); chain_equal: one call under a chain mask is the twin's O and LSE bit for bit
              (profiles/tree_gpu.log).
--accept        with --tree N[,N...]: the WRITE side of a speculative step, a mode of its own over the decode shapes
              with N draft nodes per sequence.  One line per shape and cache form (as under --sinks: --kv fp8, --paged), every figure
              per N, [median, min, max] over --repeats ALTERNATED windows of --steps calls.  The draft is a heap-shaped binary tree, the
              accepted path its last leaf's (depth + 1 nodes); the caches hold the appended draft.
              accept_ms    kv_cache_accept* of that path: one launch, indices and count read on the device
              reappend_ms  the route without it, its device side only: an index gather of the accepted rows out of K_new / V_new and
                           kv_cache_append_varlen* (with --rope: of Q too, and rope_cache_append_varlen*) at the rewound lengths.  The
                           path's length is taken from the host here and nothing is read back, which flatters this route: an engine
                           learns the path on the host, a synchronisation per step
              accept_ratio = accept_ms / reappend_ms (medians); accept_equals_reappend: the two routes leave the same bytes in the
                           whole cache (with --rope: the draft appended with pos_offsets = the depths)
              rope_append_ms, rope_pos_ms  rope_cache_append* of the N rows without and with pos_offsets = the tree's depths, alternated
              rope_pos_ratio = rope_pos_ms / rope_append_ms (medians); twin_span = max / min of rope_append_ms's own windows: the
                           ratio to hold it against (profiles/spec_step_gpu.log).
--cascade       shared-prefix decode (flash_attention_cascade_decode*) beside flash_attention_decode* on the same logical
              problem: a mode of its own over CASCADE_SHAPES (B sequences, a shared prefix of Ls keys, suffixes of Lu keys each).  One
              line per shape and cache form ("bf16", with --kv fp8 "fp8", with --paged "paged<page>" and "paged<page>_fp8").  Contiguous: the
              decode call reads caches [B, Hkv, Ls + Lu, d] that each hold a copy of the prefix; paged: the decode call's block table names
              the shared pages in every row, the cascade call gets the same pool with shared_table and the suffix columns of that table.
              The two calls share Q, the lengths, is_causal and the output type, each has its O and workspace, and they are timed
              ALTERNATED, --repeats windows of --steps calls each, after the usual priming:
              decode_ms   flash_attention_decode* under its own plan: [median, min, max] of its windows
              cascade_ms  flash_attention_cascade_decode* under the plan in "splits" = [shared, unique], likewise
              ratio = decode_ms / cascade_ms (medians); rows_ratio: the K/V rows per K/V head the two read by their grids, B (Ls + Lu) over
              ceil(B G Sq / rows_per_block) Ls + B Lu; max_diff: the largest |O_cascade - O_decode| of one call each (bf16 outputs).
              With --splits s:u[,s:u...]: the forced sweep, one line per (shape, form, pair) (profiles/cascade_gpu.log).
--mla           MLA decode (flash_attention_mla_decode*) beside the same problem from torch ops: a mode of its own over
              MLA_SHAPES -- H 16 and 128 x (B, L) = (1, 32768), (32, 8192), (128, 4096) at Sq = 1, and two H = 64 shapes with mla_ms only --
              on a latent cache [B, L, 576] bf16 with every sequence full; bf16 in and out, scale 576 ** -0.5, the library's own plan.
              The two are timed ALTERNATED, --repeats windows of --steps calls each (the log: five of 100), after the usual priming:
              mla_ms      one flash_attention_mla_decode call (O and the workspace given): [median, min, max] of its windows
              torch_ms    bf16 bmm, fp32 softmax, bf16 bmm on the contiguous cache, likewise; speedup = torch_ms / mla_ms (medians)
              kv_tbps     the cache's bytes (B L 1152) / mla_ms; kv_MB those bytes (below the 256 MiB Infinity Cache the figure is the cache's)
              tflops      2 (576 + 512) MACs per (row, key) / mla_ms
              hbm_bound_ms   one read of the cache at 6.3 TB/s;  mfma_bound_ms  the busiest wave's MFMA count per (row block, key tile) --
                          36 for the scores, 16 per 16-row tile for the P.V product with its lo half -- at 16 cycles each and 1.9 GHz, the
                          workgroups spread over min(256, grid) CUs
              max_diff_vs_torch  the largest difference of one result each (bf16 outputs)
              With --paged a,b: paged_ms[page] / paged_ratio[page], the same data in pages behind a shuffled table.  With --splits
              a,b,c: the forced sweep, one line per (shape, split count) with mla_ms only; --no-cross: no torch route
              (profiles/mla_decode_gpu.log).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [  # name, B, H, Hkv, Sq, Sk, d, ragged
    ("single_32k", 1, 32, 8, 1, 32768, 128, False),
    ("single_128k", 1, 32, 8, 1, 131072, 128, False),
    ("batch8_8k", 8, 32, 8, 1, 8192, 128, False),
    ("batch64_4k", 64, 64, 8, 1, 4096, 128, False),
    ("mha_16k", 4, 32, 32, 1, 16384, 128, False),
    ("spec4_32k", 8, 32, 8, 4, 32768, 128, False),
    ("d64_16k", 8, 32, 8, 1, 16384, 64, False),
    ("ragged", 16, 32, 8, 1, 32768, 128, True),
]
# run only when named: a short cache under a single sequence (how short a split may usefully be; single_128 and single_4k are also the
# yardsticks of --window 128,4096 on the long single-sequence shapes: un-windowed caches of the window's size)
EXTRA = [("single_2k", 1, 32, 8, 1, 2048, 128, False), ("single_4k", 1, 32, 8, 1, 4096, 128, False),
         ("single_128", 1, 32, 8, 1, 128, 128, False)]


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


EXTEND_SHAPES = [  # name, B, H, Hkv, Sq, prefixes, d
    ("chunk512_8k", 1, 32, 8, 512, [8192], 128),
    ("chunk512_32k", 1, 32, 8, 512, [32768], 128),
    ("chunk2048_0", 1, 32, 8, 2048, [0], 128),
    ("chunk64_32k", 1, 32, 8, 64, [32768], 128),
    ("batch8_ragged", 8, 32, 8, 512, [1024 + (32768 - 1024) * b // 7 for b in range(8)], 128),
    ("d64_chunk512_8k", 1, 32, 8, 512, [8192], 64),
]
# with --window (or when named): a long chunk whose length is, and one whose length is not, a multiple of rows_per_block
EXTEND_WINDOW_SHAPES = [
    ("chunk1024_32k", 1, 32, 8, 1024, [32768], 128),
    ("chunk1000_32k", 1, 32, 8, 1000, [32768], 128),
]


def extend_main(args, fa, dev):
    import torch
    f8 = torch.float8_e4m3fn
    wins = [int(x) for x in (args.window or "").split(",") if x]
    shapes = EXTEND_SHAPES + (EXTEND_WINDOW_SHAPES if wins else [])
    if args.shape:
        unknown = set(args.shape) - {x[0] for x in EXTEND_SHAPES + EXTEND_WINDOW_SHAPES}
        if unknown:
            raise SystemExit(f"unknown --extend shape(s): {sorted(unknown)}")
        shapes = [x for x in EXTEND_SHAPES + EXTEND_WINDOW_SHAPES if x[0] in args.shape]
    windows = lambda call, steps=None: sorted(timed(call, steps or args.steps, args.warmup) for _ in range(args.repeats))
    stats = lambda key, v: {key: round(statistics.median(v), 5), key + "_min": round(v[0], 5), key + "_max": round(v[-1], 5)}
    primed = False
    for name, B, H, Hkv, Sq, prefixes, d in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        lens = [p + Sq for p in prefixes]
        Sk = -(-max(lens) // 256) * 256                     # the capacity: whole pages of every --paged size
        Q = torch.randn(B, H, Sq, d, device=dev, generator=g).to(torch.bfloat16)
        K, V = (torch.randn(B, Hkv, Sk, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        O = torch.empty(B, H, Sq, d, device=dev, dtype=torch.bfloat16)
        base = {"shape": name, "B": B, "H": H, "Hkv": Hkv, "Sq": Sq, "prefix": prefixes if B > 1 else prefixes[0], "capacity": Sk, "d": d,
                "io": "bfloat16", "repeats": args.repeats, "steps": args.steps}

        def extend_call(Kc, Vc, table, kw, ns=0, W=0):
            plan = fa.extend_plan(B, H, Hkv, Sq, Sk, d, fa.FA_DTYPE_BF16, ns, window=W)
            ws = torch.empty(max(fa.decode_workspace_size(B, H, Sq, d, plan["num_splits"]), 16), dtype=torch.uint8, device=dev)
            kw = dict(kw, window=W) if W else kw
            front, paged = (fa.flash_attention_extend_window, fa.flash_attention_extend_paged_window) if W else (
                fa.flash_attention_extend, fa.flash_attention_extend_paged)
            if table is None:
                return plan, lambda: front(Q, Kc, Vc, lens_d, is_causal=True, O=O, workspace=ws, num_splits=ns, **kw)
            return plan, lambda: paged(Q, Kc, Vc, table, lens_d, is_causal=True, O=O, workspace=ws, num_splits=ns, **kw)

        def windowed(call_of, key):
            """{key_ms: {W: median}, key_ms_min / _max, window_splits}: the windowed call per --window value"""
            out = {key + "_ms": {}, key + "_ms_min": {}, key + "_ms_max": {}, "window_splits": {}}
            for W in wins:
                plan, call = call_of(W)
                v = windows(call)
                out[key + "_ms"][str(W)], out[key + "_ms_min"][str(W)], out[key + "_ms_max"][str(W)] = (
                    round(statistics.median(v), 5), round(v[0], 5), round(v[-1], 5))
                out["window_splits"][str(W)] = plan["num_splits"]
            return out

        def prime(call):
            nonlocal primed
            if not primed:   # >= 1 s of calls before the first timed window
                t = 0.0
                while t < 1000.0:
                    t += timed(call, 20, 0) * 20
                primed = True

        if args.splits:
            for ns in [int(x) for x in args.splits.split(",")]:
                if ns > -(-Sk // 128):
                    continue
                plan, call = extend_call(K, V, None, {}, ns)
                prime(call)
                line = dict({"shape": name, "forced_splits": ns, "grid": plan["grid"]}, **stats("extend_ms", windows(call)))
                if wins:
                    line.update(windowed(lambda W: extend_call(K, V, None, {}, ns, W), "extend_window"))
                    del line["window_splits"]
                print(json.dumps(line), flush=True)
            del Q, K, V, O
            torch.cuda.empty_cache()
            continue

        def sliced_call(Kc, Vc, table, kw):
            # flash_attention_decode* in 16-row slices: slice j holds the query rows [16 j, 16 j + 16) and sees kv_lens - Sq + its last row + 1
            Os = torch.empty_like(O)
            cuts = [(j, min(j + 16, Sq)) for j in range(0, Sq, 16)]
            slens = [(lens_d - Sq + e).contiguous() for _, e in cuts]
            ns = fa.decode_plan(B, H, Hkv, 16, Sk, d, fa.FA_DTYPE_BF16, 0)["num_splits"]
            ws = torch.empty(max(fa.decode_workspace_size(B, H, 16, d, ns), 16), dtype=torch.uint8, device=dev)

            def call():
                for (a, e), L in zip(cuts, slens):
                    if table is None:
                        fa.flash_attention_decode(Q[:, :, a:e], Kc, Vc, L, is_causal=True, O=Os[:, :, a:e], workspace=ws, **kw)
                    else:
                        fa.flash_attention_decode_paged(Q[:, :, a:e], Kc, Vc, table, L, is_causal=True, O=Os[:, :, a:e], workspace=ws, **kw)
            return Os, call

        def pair_call():
            # the prefill kernels: not causal over the prefix, causal (top-left = bottom-right: square) over the chunk's own keys
            Op = torch.empty(B, H, Sq, d, device=dev, dtype=torch.float32)

            def one(b0, b1, p):
                q = Q[b0:b1]
                o2, l2 = fa.flash_attention(q, K[b0:b1, :, p:p + Sq], V[b0:b1, :, p:p + Sq], is_causal=True, out_dtype=torch.float32, return_lse=True)
                if p == 0:
                    Op[b0:b1] = o2
                    return
                o1, l1 = fa.flash_attention(q, K[b0:b1, :, :p], V[b0:b1, :, :p], out_dtype=torch.float32, return_lse=True)
                w1 = torch.sigmoid(l1 - l2)[..., None]
                Op[b0:b1] = o1 * w1 + o2 * (1 - w1)

            def call():
                if len(set(prefixes)) == 1:
                    one(0, B, prefixes[0])
                else:
                    for b, p in enumerate(prefixes):
                        one(b, b + 1, p)
            return Op, call

        forms = [("bf16", False, 0)] + ([("fp8", True, 0)] if args.kv == "fp8" else [])
        for page in (int(x) for x in (args.paged or "").split(",") if x):
            forms += [(f"paged{page}", False, page)] + ([(f"paged{page}_fp8", True, page)] if args.kv == "fp8" else [])
        if args.kv == "fp8":
            quant = lambda T: (lambda ds: ((T.float() / ds[None, :, None, None]).clamp(-448, 448).to(f8), ds))((T.float().abs().amax(dim=(0, 2, 3)) / 448.0).float())
            (K8, kds), (V8, vds) = quant(K), quant(V)
        for form, fp8, page in forms:
            Kc, Vc, table = (K8, V8, None) if fp8 else (K, V, None)
            kw = dict(k_descale=kds, v_descale=vds) if fp8 else {}
            line = dict(base, form=form)
            if page:
                n = Sk // page
                perm = torch.randperm(B * n, device=dev, generator=g)
                table = perm.reshape(B, n).to(torch.int32)
                pools = []
                for T in (Kc, Vc):
                    T = T.view(torch.uint8) if fp8 else T      # (pages are moved as bytes)
                    pool = torch.empty(B * n, Hkv, page, d, device=dev, dtype=T.dtype)
                    pool[perm] = T.view(B, Hkv, n, page, d).transpose(1, 2).reshape(B * n, Hkv, page, d)
                    pools.append(pool.view(f8) if fp8 else pool)
                Kc, Vc = pools
                tl = table.long()
                gather = lambda: [P.view(torch.uint8 if fp8 else P.dtype)[tl].permute(0, 2, 1, 3, 4).reshape(B, Hkv, Sk, d) for P in (Kc, Vc)]
                if not wins:
                    line.update(stats("gather_ms", windows(gather, max(10, args.steps // 10))))
            if fp8 and not wins:
                deq = lambda: [(T.to(torch.bfloat16) * ds[None, :, None, None].to(torch.bfloat16)) for T, ds in ((K8, kds), (V8, vds))]
                line.update(stats("dequantise_ms", windows(deq, max(10, args.steps // 10))))
            plan, call = extend_call(Kc, Vc, table, kw)
            prime(call)
            line.update(stats("extend_ms", windows(call)))
            line.update(splits=plan["num_splits"], row_blocks=plan["row_blocks"], rows_per_block=plan["rows_per_block"], grid=plan["grid"])
            if wins:   # the windowed call beside the un-windowed one; the comparison routes are not timed
                line.update(windowed(lambda W: extend_call(Kc, Vc, table, kw, 0, W), "extend_window"))
                print(json.dumps(line), flush=True)
                continue
            Os, scall = sliced_call(Kc, Vc, table, kw)
            line.update(stats("sliced_decode_ms", windows(scall, max(3, args.steps // 20))))
            line["extend_vs_sliced_max_abs"] = round((O.float() - Os.float()).abs().max().item(), 6)
            line["sliced_over_extend"] = round(line["sliced_decode_ms"] / line["extend_ms"], 2)
            if form == "bf16":
                Op, pcall = pair_call()
                line.update(stats("prefill_pair_ms", windows(pcall, max(10, args.steps // 10))))
                line["pair_vs_extend_max_abs"] = round((O.float() - Op).abs().max().item(), 6)
                line["pair_over_extend"] = round(line["prefill_pair_ms"] / line["extend_ms"], 2)
                del Op
            print(json.dumps(line), flush=True)
            del Os
        del Q, K, V, O
        torch.cuda.empty_cache()


def varlen_shapes():
    """name, d, [(rows, prefix)] per sequence, in batch order; sequences of one row count are neighbours, so that the grouped calls
    of `grouped_ms` take slices of the batch"""
    out = []
    for d in (128, 64):
        s = "" if d == 128 else "d64_"
        out += [(s + "decode63_chunk512", d, [(1, 8192 + (32768 - 8192) * b // 62) for b in range(63)] + [(512, 8192)]),
                (s + "chunks8_64_1024", d, [(r, 1024 + (32768 - 1024) * b // 7) for b, r in enumerate((64, 128, 192, 256, 384, 512, 768, 1024))]),
                (s + "uniform8x512_8k", d, [(512, 8192)] * 8),
                (s + "decode64_16k", d, [(1, 16384 - 1)] * 64)]
    return out


def varlen_main(args, fa, dev):
    """--varlen: flash_attention_extend_varlen / _paged_varlen on mixed batches (H32 Hkv8, causal), beside what a caller does today"""
    import torch
    f8 = torch.float8_e4m3fn
    H, Hkv = 32, 8
    wins = [int(x) for x in (args.window or "").split(",") if x]
    shapes = varlen_shapes()
    if args.shape:
        unknown = set(args.shape) - {x[0] for x in shapes}
        if unknown:
            raise SystemExit(f"unknown --varlen shape(s): {sorted(unknown)}")
        shapes = [x for x in shapes if x[0] in args.shape]
    windows = lambda call, steps=None: sorted(timed(call, steps or args.steps, args.warmup) for _ in range(args.repeats))
    stats = lambda key, v: {key: round(statistics.median(v), 5), key + "_min": round(v[0], 5), key + "_max": round(v[-1], 5)}
    primed = False
    for name, d, seqs in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        B, sq = len(seqs), [r for r, _ in seqs]
        lens = [r + p for r, p in seqs]
        cu = [0]
        for r in sq:
            cu.append(cu[-1] + r)
        T = cu[-1]
        Sk = -(-max(lens) // 256) * 256                     # the capacity: whole pages of every --paged size
        Q = torch.randn(T, H, d, device=dev, generator=g).to(torch.bfloat16)
        K, V = (torch.randn(B, Hkv, Sk, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
        Kn, Vn = (torch.randn(T, Hkv, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
        cu_d, lens_d = torch.tensor(cu, dtype=torch.int32, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev)
        O = torch.zeros(T, H, d, device=dev, dtype=torch.bfloat16)
        # the groups of today's calls: runs of one row count -> (first sequence, one past the last, rows)
        groups = []
        for b, r in enumerate(sq):
            if groups and groups[-1][2] == r:
                groups[-1][1] = b + 1
            else:
                groups.append([b, b + 1, r])
        base = {"shape": name, "B": B, "H": H, "Hkv": Hkv, "d": d, "totalQ": T, "rows": sq if len(set(sq)) > 1 else sq[0],
                "kv_len_min": min(lens), "kv_len_max": max(lens), "capacity": Sk, "io": "bfloat16", "repeats": args.repeats, "steps": args.steps}

        def varlen_call(Kc, Vc, table, kw, ns=0, W=0):
            plan = fa.extend_varlen_plan(B, H, Hkv, T, Sk, d, fa.FA_DTYPE_BF16, ns, window=W)
            ws = torch.empty(max(fa.decode_workspace_size(1, H, T, d, plan["num_splits"]), 16), dtype=torch.uint8, device=dev)
            kw = dict(kw, window=W) if W else kw
            front, paged = (fa.flash_attention_extend_varlen_window, fa.flash_attention_extend_paged_varlen_window) if W else (
                fa.flash_attention_extend_varlen, fa.flash_attention_extend_paged_varlen)
            if table is None:
                return plan, lambda: front(Q, Kc, Vc, cu_d, lens_d, is_causal=True, O=O, workspace=ws, num_splits=ns, **kw)
            return plan, lambda: paged(Q, Kc, Vc, table, cu_d, lens_d, is_causal=True, O=O, workspace=ws, num_splits=ns, **kw)

        def prime(call):
            nonlocal primed
            if not primed:   # >= 1 s of calls before the first timed window
                t = 0.0
                while t < 1000.0:
                    t += timed(call, 20, 0) * 20
                primed = True

        def windowed(call_of, key):
            """{key_ms: {W: median}, key_ms_min / _max, window_splits}: the windowed call per --window value"""
            out = {key + "_ms": {}, key + "_ms_min": {}, key + "_ms_max": {}, "window_splits": {}}
            for W in wins:
                plan, call = call_of(W)
                v = windows(call)
                out[key + "_ms"][str(W)], out[key + "_ms_min"][str(W)], out[key + "_ms_max"][str(W)] = (
                    round(statistics.median(v), 5), round(v[0], 5), round(v[-1], 5))
                out["window_splits"][str(W)] = plan["num_splits"]
            return out

        if args.splits:
            for ns in [int(x) for x in args.splits.split(",")]:
                if ns > -(-Sk // 128):
                    continue
                plan, call = varlen_call(K, V, None, {}, ns)
                prime(call)
                line = dict({"shape": name, "forced_splits": ns, "grid": plan["grid"]}, **stats("varlen_ms", windows(call)))
                if wins:
                    line.update(windowed(lambda W: varlen_call(K, V, None, {}, ns, W), "varlen_window"))
                    del line["window_splits"]
                print(json.dumps(line), flush=True)
            del Q, K, V, O, Kn, Vn
            torch.cuda.empty_cache()
            continue

        def regroup_calls():
            """the copies between the engine's token-major tensors and the [Bg, H, rows, d] tensors of the grouped calls: Q in, O back"""
            Qg = [torch.empty(b1 - b0, H, r, d, device=dev, dtype=torch.bfloat16) for b0, b1, r in groups]
            Og = [torch.empty_like(q) for q in Qg]
            Oback = torch.empty_like(O)

            def call():
                for (b0, b1, r), q, o in zip(groups, Qg, Og):
                    q.copy_(Q[cu[b0]:cu[b1]].view(b1 - b0, r, H, d).transpose(1, 2))
                    Oback[cu[b0]:cu[b1]].view(b1 - b0, r, H, d).copy_(o.transpose(1, 2))
            call()
            return Qg, Og, call

        def grouped_call(Qg, Og, Kc, Vc, table, kw):
            """one flash_attention_decode* for the rows <= 16, one flash_attention_extend* per other row count, on pre-grouped tensors"""
            calls = []
            for (b0, b1, r), q, o in zip(groups, Qg, Og):
                n = b1 - b0
                L = lens_d[b0:b1].contiguous()
                front = "flash_attention_decode" if r <= fa.FA_DECODE_MAX_Q else "flash_attention_extend"
                plan = (fa.decode_plan if r <= fa.FA_DECODE_MAX_Q else fa.extend_plan)(n, H, Hkv, r, Sk, d, fa.FA_DTYPE_BF16, 0)
                ws = torch.empty(max(fa.decode_workspace_size(n, H, r, d, plan["num_splits"]), 16), dtype=torch.uint8, device=dev)
                if table is None:
                    calls.append(lambda f=getattr(fa, front), q=q, o=o, L=L, ws=ws, b0=b0, b1=b1:
                                 f(q, Kc[b0:b1], Vc[b0:b1], L, is_causal=True, O=o, workspace=ws, **kw))
                else:
                    calls.append(lambda f=getattr(fa, front + "_paged"), q=q, o=o, L=L, ws=ws, t=table[b0:b1]:
                                 f(q, Kc, Vc, t, L, is_causal=True, O=o, workspace=ws, **kw))
            return lambda: [c() for c in calls]

        def append_calls(Kc, Vc, table, kw):
            """(the ragged append, today's appends: one uniform call per group on pre-grouped new rows) into copies of the cache form"""
            Kw, Vw = Kc.clone(), Vc.clone()
            Kg = [Kn[cu[b0]:cu[b1]].view(b1 - b0, r, Hkv, d).transpose(1, 2).contiguous() for b0, b1, r in groups]
            Vg = [Vn[cu[b0]:cu[b1]].view(b1 - b0, r, Hkv, d).transpose(1, 2).contiguous() for b0, b1, r in groups]
            Lg = [lens_d[b0:b1].contiguous() for b0, b1, _ in groups]
            if table is None:
                ragged = lambda: fa.kv_cache_append_varlen(Kn, Vn, Kw, Vw, cu_d, lens_d, **kw)
                today = lambda: [fa.kv_cache_append(k, v, Kw[b0:b1], Vw[b0:b1], L, **kw) for (b0, b1, _), k, v, L in zip(groups, Kg, Vg, Lg)]
            else:
                ragged = lambda: fa.kv_cache_append_paged_varlen(Kn, Vn, Kw, Vw, table, cu_d, lens_d, **kw)
                today = lambda: [fa.kv_cache_append_paged(k, v, Kw, Vw, table[b0:b1], L, **kw) for (b0, b1, _), k, v, L in zip(groups, Kg, Vg, Lg)]
            return ragged, today

        forms = [("bf16", False, 0)] + ([("fp8", True, 0)] if args.kv == "fp8" else [])
        for page in (int(x) for x in (args.paged or "").split(",") if x):
            forms += [(f"paged{page}", False, page)] + ([(f"paged{page}_fp8", True, page)] if args.kv == "fp8" else [])
        if args.kv == "fp8":
            def quant(Tn):
                ds = (Tn.float().abs().amax(dim=(0, 2, 3)) / 448.0).float()
                T8 = torch.empty(Tn.shape, dtype=f8, device=dev)
                for b in range(B):     # (a batch entry at a time: no fp32 copy of the whole cache)
                    T8[b] = (Tn[b].float() / ds[:, None, None]).clamp(-448, 448).to(f8)
                return T8, ds
            (K8, kds), (V8, vds) = quant(K), quant(V)
        if not wins:
            Qg, Og, rcall = regroup_calls()
            regroup = stats("regroup_ms", windows(rcall))
        else:
            Qg = Og = None
        for form, fp8, page in forms:
            Kc, Vc, table = (K8, V8, None) if fp8 else (K, V, None)
            kw = dict(k_descale=kds, v_descale=vds) if fp8 else {}
            line = dict(base, form=form)
            if page:
                n = Sk // page
                perm = torch.randperm(B * n, device=dev, generator=g)
                table = perm.reshape(B, n).to(torch.int32)
                pools = []
                for Tn in (Kc, Vc):
                    Tn = Tn.view(torch.uint8) if fp8 else Tn      # (pages are moved as bytes)
                    pool = torch.empty(B * n, Hkv, page, d, device=dev, dtype=Tn.dtype)
                    pool[perm] = Tn.view(B, Hkv, n, page, d).transpose(1, 2).reshape(B * n, Hkv, page, d)
                    pools.append(pool.view(f8) if fp8 else pool)
                Kc, Vc = pools
            plan, call = varlen_call(Kc, Vc, table, kw)
            prime(call)
            line.update(stats("varlen_ms", windows(call)))
            line.update(splits=plan["num_splits"], row_blocks_bound=plan["row_blocks"], rows_per_block=plan["rows_per_block"], grid=plan["grid"],
                        row_blocks_real=sum(-(-(H // Hkv) * r // plan["rows_per_block"]) for r in sq))
            if wins:   # the windowed call beside the un-windowed one; the comparison routes are not timed
                line.update(windowed(lambda W: varlen_call(Kc, Vc, table, kw, 0, W), "varlen_window"))
                print(json.dumps(line), flush=True)
                continue
            gcall = grouped_call(Qg, Og, Kc, Vc, table, kw)
            line.update(stats("grouped_ms", windows(gcall)))
            line["grouped_calls"] = len(groups)
            line.update(regroup)
            worst = max(((O[cu[b0]:cu[b1]].view(b1 - b0, r, H, d).transpose(1, 2).float() - o.float()).abs().max().item()
                         for (b0, b1, r), o in zip(groups, Og)))
            line["varlen_vs_grouped_max_abs"] = round(worst, 6)
            line["varlen_over_grouped"] = round(line["varlen_ms"] / line["grouped_ms"], 3)
            line["varlen_over_grouped_and_regroup"] = round(line["varlen_ms"] / (line["grouped_ms"] + line["regroup_ms"]), 3)
            if len(groups) == 1:   # a uniform batch: grouped_ms IS the uniform call of the same problem -- the cost of being ragged
                line["extend_ms" if sq[0] > fa.FA_DECODE_MAX_Q else "ms"] = line["grouped_ms"]
            ragged, today = append_calls(Kc, Vc, table, kw)
            line.update(stats("append_varlen_ms", windows(ragged)))
            line.update(stats("append_ms", windows(today)))
            print(json.dumps(line), flush=True)
        del Q, K, V, O, Kn, Vn, Qg, Og
        if args.kv == "fp8":
            del K8, V8
        torch.cuda.empty_cache()


def sinks_main(args, fa, dev):
    """--sinks: every shape of the chosen family with and without ``sinks=``, alternated"""
    import torch
    f8 = torch.float8_e4m3fn
    wins = [0] + [int(x) for x in (args.window or "").split(",") if x]
    pages = [int(x) for x in (args.paged or "").split(",") if x]
    if args.varlen:
        cases = [(name, d, 32, 8, [r for r, _ in seqs], [r + p for r, p in seqs]) for name, d, seqs in varlen_shapes()]
    elif args.extend:
        cases = [(name, d, H, Hkv, [Sq] * B, [p + Sq for p in prefixes]) for name, B, H, Hkv, Sq, prefixes, d in EXTEND_SHAPES + EXTEND_WINDOW_SHAPES]
    else:
        cases = [(name, d, H, Hkv, [Sq] * B, [1024 + (Sk - 1024) * b // (B - 1) for b in range(B)] if ragged else [Sk] * B)
                 for name, B, H, Hkv, Sq, Sk, d, ragged in SHAPES + EXTRA]
    if args.shape:
        unknown = set(args.shape) - {c[0] for c in cases}
        if unknown:
            raise SystemExit(f"unknown shape(s): {sorted(unknown)}")
        cases = [c for c in cases if c[0] in args.shape]
    elif not args.varlen:
        cases = [c for c in cases if c[0] not in {x[0] for x in EXTRA + EXTEND_WINDOW_SHAPES}]
    family = "varlen" if args.varlen else "extend" if args.extend else "decode"
    plan_of = {"decode": fa.decode_plan, "extend": fa.extend_plan, "varlen": fa.extend_varlen_plan}[family]
    primed = False
    for name, d, H, Hkv, sq, lens in cases:
        g = torch.Generator(device=dev).manual_seed(0)
        B, T = len(sq), sum(sq)
        Sk = -(-max(lens) // 256) * 256 if family != "decode" else max(lens)
        Q = torch.randn((T, H, d) if family == "varlen" else (B, H, sq[0], d), device=dev, generator=g).to(torch.bfloat16)
        K, V = (torch.randn(B, Hkv, Sk, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        cu = [0]
        for r in sq:
            cu.append(cu[-1] + r)
        cu_d = torch.tensor(cu, dtype=torch.int32, device=dev)
        O = torch.zeros_like(Q)
        # logits around the LSE of a row of N(0, 1) data: ln(keys) + 1/2 for the longest sequence, spread by +-2 over the heads
        sinks = (torch.linspace(-2.0, 2.0, H) + torch.log(torch.tensor(float(max(lens)))) + 0.5).to(dev)
        forms = [("bf16", False, 0)] + ([("fp8", True, 0)] if args.kv == "fp8" else [])
        for page in pages:
            if Sk % page == 0:
                forms += [(f"paged{page}", False, page)] + ([(f"paged{page}_fp8", True, page)] if args.kv == "fp8" else [])
        if args.kv == "fp8":
            def quant(Tn):
                ds = (Tn.float().abs().amax(dim=(0, 2, 3)) / 448.0).float()
                T8 = torch.empty(Tn.shape, dtype=f8, device=dev)
                for b in range(B):     # (a batch entry at a time: no fp32 copy of the whole cache)
                    T8[b] = (Tn[b].float() / ds[:, None, None]).clamp(-448, 448).to(f8)
                return T8, ds
            (K8, kds), (V8, vds) = quant(K), quant(V)
        for form, fp8, page in forms:
            Kc, Vc, table = (K8, V8, None) if fp8 else (K, V, None)
            kw = dict(k_descale=kds, v_descale=vds) if fp8 else {}
            if page:
                n = Sk // page
                perm = torch.randperm(B * n, device=dev, generator=g)
                table = perm.reshape(B, n).to(torch.int32)
                pools = []
                for Tn in (Kc, Vc):
                    Tn = Tn.view(torch.uint8) if fp8 else Tn      # (pages are moved as bytes)
                    pool = torch.empty(B * n, Hkv, page, d, device=dev, dtype=Tn.dtype)
                    pool[perm] = Tn.view(B, Hkv, n, page, d).transpose(1, 2).reshape(B * n, Hkv, page, d)
                    pools.append(pool.view(f8) if fp8 else pool)
                Kc, Vc = pools
            front = getattr(fa, {"decode": "flash_attention_decode", "extend": "flash_attention_extend", "varlen": "flash_attention_extend"}[family]
                            + ("_paged" if page else "") + ("_varlen" if family == "varlen" else "") + ("" if family == "decode" else "_window"))
            head = [Q, Kc, Vc] + ([table] if page else []) + ([cu_d] if family == "varlen" else []) + [lens_d]
            line = {"shape": name, "form": form, "splits": {}, "ms": {}, "sink_ms": {}, "sink_ratio": {}}
            for W in wins:
                plan = plan_of(B, H, Hkv, T if family == "varlen" else sq[0], Sk, d, fa.FA_DTYPE_BF16, 0, window=W)
                ws = torch.empty(max(fa.decode_workspace_size(1 if family == "varlen" else B, H, T if family == "varlen" else sq[0], d,
                                                              plan["num_splits"]), 16), dtype=torch.uint8, device=dev)
                common = dict(kw, is_causal=family != "decode", O=O, workspace=ws, window=W)
                plain = lambda: front(*head, **common)
                sunk = lambda: front(*head, sinks=sinks, **common)
                if not primed:   # >= 1 s of calls before the first timed window
                    t = 0.0
                    while t < 1000.0:
                        t += timed(plain, 50, 0) * 50
                    primed = True
                a, b = [], []
                for _ in range(args.repeats):
                    a.append(timed(plain, args.steps, args.warmup))
                    b.append(timed(sunk, args.steps, args.warmup))
                a, b = sorted(a), sorted(b)
                line["splits"][str(W)] = plan["num_splits"]
                line["ms"][str(W)] = [round(x, 5) for x in (statistics.median(a), a[0], a[-1])]
                line["sink_ms"][str(W)] = [round(x, 5) for x in (statistics.median(b), b[0], b[-1])]
                line["sink_ratio"][str(W)] = round(statistics.median(b) / statistics.median(a), 4)
            print(json.dumps(line), flush=True)
        del Q, K, V, O
        if args.kv == "fp8":
            del K8, V8
        torch.cuda.empty_cache()


CASCADE_SHAPES = [  # name, B, H, Hkv, Sq, Ls, Lu, d
    ("cascade_b8", 8, 32, 8, 1, 8192, 256, 128),
    ("cascade_b32", 32, 32, 8, 1, 8192, 256, 128),
    ("cascade_b32_spec4", 32, 32, 8, 4, 8192, 256, 128),
    ("cascade_b2_short", 2, 32, 8, 1, 128, 256, 128),      # sharing cannot pay: two sequences, one tile of prefix
]


def cascade_main(args, fa, dev):
    """--cascade: flash_attention_cascade_decode* beside flash_attention_decode* on the same logical problem, alternated"""
    import torch
    f8 = torch.float8_e4m3fn
    pages = [int(x) for x in (args.paged or "").split(",") if x]
    sweep = [tuple(int(n) for n in pair.split(":")) for pair in (args.splits or "").split(",") if pair] or [(0, 0)]
    shapes = CASCADE_SHAPES
    if args.shape:
        unknown = set(args.shape) - {x[0] for x in CASCADE_SHAPES}
        if unknown:
            raise SystemExit(f"unknown --cascade shape(s): {sorted(unknown)}")
        shapes = [x for x in CASCADE_SHAPES if x[0] in args.shape]
    primed = False
    for name, B, H, Hkv, Sq, Ls, Lu, d in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g).to(torch.bfloat16)
        Q, Ks, Vs, Ku, Vu = rnd(B, H, Sq, d), rnd(Hkv, Ls, d), rnd(Hkv, Ls, d), rnd(B, Hkv, Lu, d), rnd(B, Hkv, Lu, d)
        lens_u = torch.full((B,), Lu, dtype=torch.int32, device=dev)
        lens_all = torch.full((B,), Ls + Lu, dtype=torch.int32, device=dev)
        sl = torch.tensor([Ls], dtype=torch.int32, device=dev)
        Od, Oc = (torch.empty(B, H, Sq, d, device=dev, dtype=torch.bfloat16) for _ in range(2))
        forms = [("bf16", False, 0)] + ([("fp8", True, 0)] if args.kv == "fp8" else [])
        for page in pages:
            if Ls % page == 0 and Lu % page == 0:
                forms += [(f"paged{page}", False, page)] + ([(f"paged{page}_fp8", True, page)] if args.kv == "fp8" else [])
        kw = {}
        if args.kv == "fp8":      # one descale pair per K/V head for both parts
            kds, vds = ((torch.maximum(s.float().abs().amax(dim=(1, 2)), u.float().abs().amax(dim=(0, 2, 3))) / 448.0).float()
                        for s, u in ((Ks, Ku), (Vs, Vu)))
            q8 = lambda t, ds, dim: (t.float() / ds.view([-1 if i == dim else 1 for i in range(t.dim())])).clamp(-448, 448).to(f8)
            Ks8, Vs8, Ku8, Vu8 = q8(Ks, kds, 0), q8(Vs, vds, 0), q8(Ku, kds, 1), q8(Vu, vds, 1)
        rpb = fa.cascade_plan(B, H, Hkv, Sq, Ls, Lu, d)["shared"]["rows_per_block"]
        rows_ratio = round(B * (Ls + Lu) / (-(-B * (H // Hkv) * Sq // rpb) * Ls + B * Lu), 3)
        for form, fp8, page in forms:
            s_k, s_v, u_k, u_v = (Ks8, Vs8, Ku8, Vu8) if fp8 else (Ks, Vs, Ku, Vu)
            kw = dict(k_descale=kds, v_descale=vds) if fp8 else {}
            if page:
                ns_p, nu_p = Ls // page, Lu // page
                perm = torch.randperm(ns_p + B * nu_p, device=dev, generator=g)
                shared_table = perm[:ns_p].to(torch.int32).contiguous()
                suffix_table = perm[ns_p:].reshape(B, nu_p).to(torch.int32)
                full_table = torch.cat([shared_table[None].expand(B, -1), suffix_table], 1).contiguous()
                pools = []
                for s_t, u_t in ((s_k, u_k), (s_v, u_v)):
                    s_t, u_t = (t.view(torch.uint8) if fp8 else t for t in (s_t, u_t))      # (pages are moved as bytes)
                    pool = torch.empty(ns_p + B * nu_p, Hkv, page, d, device=dev, dtype=s_t.dtype)
                    pool[perm[:ns_p]] = s_t.view(Hkv, ns_p, page, d).transpose(0, 1)
                    pool[perm[ns_p:]] = u_t.view(B, Hkv, nu_p, page, d).transpose(1, 2).reshape(B * nu_p, Hkv, page, d)
                    pools.append(pool.view(f8) if fp8 else pool)
                decode_head, decode_front = [Q, pools[0], pools[1], full_table, lens_all], fa.flash_attention_decode_paged
                cascade_head = [Q, pools[0], pools[1], shared_table, full_table[:, ns_p:], sl, lens_u]
                cascade_front = fa.flash_attention_cascade_decode_paged
            else:
                cat = lambda s_t, u_t: torch.cat([s_t[None].expand(B, -1, -1, -1).view(torch.uint8 if fp8 else s_t.dtype),
                                                  u_t.view(torch.uint8 if fp8 else u_t.dtype)], 2).contiguous()
                Kd, Vd = cat(s_k, u_k), cat(s_v, u_v)
                if fp8:
                    Kd, Vd = Kd.view(f8), Vd.view(f8)
                decode_head, decode_front = [Q, Kd, Vd, lens_all], fa.flash_attention_decode
                cascade_head, cascade_front = [Q, s_k, s_v, u_k, u_v, sl, lens_u], fa.flash_attention_cascade_decode
            dplan = fa.decode_plan(B, H, Hkv, Sq, Ls + Lu, d, fa.FA_DTYPE_BF16, 0)
            dws = torch.empty(max(fa.decode_workspace_size(B, H, Sq, d, dplan["num_splits"]), 16), dtype=torch.uint8, device=dev)
            decode = lambda: decode_front(*decode_head, is_causal=True, O=Od, workspace=dws, **kw)
            for pair in sweep:
                cplan = fa.cascade_plan(B, H, Hkv, Sq, Ls, Lu, d, fa.FA_DTYPE_BF16, pair)
                cws = torch.empty(fa.decode_workspace_size(B, H, Sq, d, cplan["num_splits"]), dtype=torch.uint8, device=dev)
                cascade = lambda: cascade_front(*cascade_head, is_causal=True, O=Oc, workspace=cws, num_splits=pair, **kw)
                if not primed:   # >= 1 s of calls before the first timed window
                    t = 0.0
                    while t < 1000.0:
                        t += timed(decode, 50, 0) * 50
                    primed = True
                a, b = [], []
                for _ in range(args.repeats):
                    a.append(timed(decode, args.steps, args.warmup))
                    b.append(timed(cascade, args.steps, args.warmup))
                a, b = sorted(a), sorted(b)
                print(json.dumps({"shape": name, "form": form, "B": B, "Sq": Sq, "Ls": Ls, "Lu": Lu,
                                  "decode_splits": dplan["num_splits"], "splits": [cplan["shared"]["num_splits"], cplan["unique"]["num_splits"]],
                                  "forced": pair != (0, 0),
                                  "decode_ms": [round(x, 5) for x in (statistics.median(a), a[0], a[-1])],
                                  "cascade_ms": [round(x, 5) for x in (statistics.median(b), b[0], b[-1])],
                                  "ratio": round(statistics.median(a) / statistics.median(b), 4), "rows_ratio": rows_ratio,
                                  "max_diff": round((Oc.float() - Od.float()).abs().max().item(), 5)}), flush=True)
            del decode_head, cascade_head
        del Q, Ks, Vs, Ku, Vu
        torch.cuda.empty_cache()


MLA_SHAPES = [  # name, B, H, Sq, L, beside torch: the latent cache is [B, L, 576] bf16, every sequence full
    ("h16_b1_32k", 1, 16, 1, 32768, True), ("h16_b32_8k", 32, 16, 1, 8192, True), ("h16_b128_4k", 128, 16, 1, 4096, True),
    ("h128_b1_32k", 1, 128, 1, 32768, True), ("h128_b32_8k", 32, 128, 1, 8192, True), ("h128_b128_4k", 128, 128, 1, 4096, True),
    # one row block where the H = 128 shapes have two: does the second block read the cache from L2 or from HBM?  mla_ms only
    ("h64_b32_8k", 32, 64, 1, 8192, False), ("h64_b128_4k", 128, 64, 1, 4096, False),
]
# (No Sq = 2 shape: at B 32, H 128, Sq 2, L 8192 the torch route's own kernels -- 256 rows per sequence against the strided views of
# the 576-wide cache -- ended in an illegal memory access on the MI355X, in torch's window, after the library's window had been
# synchronised clean.  The cause inside torch's kernels was not found, so the shape is left out, and the shapes that were not run beside
# torch before are timed without it.)
# the bounds printed beside the H = 128 figures (MI355X: about 6.3 TB/s of HBM reads are achievable; a bf16 16x16x32 MFMA takes 16
# cycles of its SIMD, and MFMA-dense loops on random data hold about 1.9 GHz under the power limit; 256 CUs)
MLA_HBM_TBPS, MLA_MFMA_CYCLES, MLA_LOADED_GHZ, MLA_CUS = 6.3, 16, 1.9, 256


def mla_main(args, fa, dev):
    """--mla: flash_attention_mla_decode* beside the same problem from torch ops, alternated"""
    import torch
    pages = [int(x) for x in (args.paged or "").split(",") if x]
    sweep = [int(n) for n in (args.splits or "").split(",") if n]
    shapes = MLA_SHAPES
    if args.shape:
        unknown = set(args.shape) - {x[0] for x in MLA_SHAPES}
        if unknown:
            raise SystemExit(f"unknown --mla shape(s): {sorted(unknown)}")
        shapes = [x for x in MLA_SHAPES if x[0] in args.shape]
    DL, D = fa.MLA_D_LATENT, fa.MLA_D_LATENT + fa.MLA_D_ROPE
    scale = D ** -0.5
    primed = False
    for name, B, H, Sq, L, beside_torch in shapes:
        beside_torch = beside_torch and not args.no_cross
        g = torch.Generator(device=dev).manual_seed(0)
        Q = torch.randn(B, H, Sq, D, device=dev, generator=g).to(torch.bfloat16)
        KV = torch.randn(B, L, D, device=dev, generator=g).to(torch.bfloat16)
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        O = torch.empty(B, H, Sq, DL, device=dev, dtype=torch.bfloat16)
        plan = fa.mla_decode_plan(B, H, Sq, L, fa.FA_DTYPE_BF16, 0)
        ws = torch.empty(max(fa.decode_workspace_size(B, H, Sq, DL, max([plan["num_splits"]] + sweep)), 16), dtype=torch.uint8, device=dev)
        mla = lambda ns=0: fa.flash_attention_mla_decode(Q, KV, lens, O=O, workspace=ws, num_splits=ns)
        q2, kt, v = Q.view(B, H * Sq, D), KV.transpose(1, 2), KV[..., :DL]

        def torch_ops():      # bf16 matmul, fp32 softmax, bf16 matmul; contiguous cache only
            p = torch.softmax(torch.bmm(q2, kt).float() * scale, -1).to(torch.bfloat16)
            return torch.bmm(p, v).view(B, H, Sq, DL)

        if not primed:   # >= 1 s of calls before the first timed window
            t = 0.0
            while t < 1000.0:
                t += timed(mla, 50, 0) * 50
            primed = True
        kv_bytes = B * L * D * 2
        # what the kernel issues: per (row block, 32-key tile) the busiest wave runs 36 score MFMAs and 16 per row tile of the block for P.V
        blocks, nrt = plan["row_blocks"], min(-(-H * Sq // 16), 4)
        wave_mfmas = B * blocks * -(-L // plan["kv_block_rows"]) * (36 + 16 * nrt)
        base = {"shape": name, "B": B, "H": H, "Sq": Sq, "L": L, "kv_MB": round(kv_bytes / 1e6, 1), "row_blocks": blocks}
        if sweep:
            for ns in sweep:
                w = sorted(timed(lambda: mla(ns), args.steps, args.warmup) for _ in range(args.repeats))
                print(json.dumps(dict(base, splits=ns, forced=True, mla_ms=[round(x, 5) for x in (statistics.median(w), w[0], w[-1])])), flush=True)
            continue
        a, b = [], []
        for _ in range(args.repeats):
            a.append(timed(mla, args.steps, args.warmup))
            if beside_torch:
                b.append(timed(torch_ops, args.steps, args.warmup))
        a, b = sorted(a), sorted(b)
        ms = statistics.median(a)
        out = dict(base, splits=plan["num_splits"], grid=plan["grid"], mla_ms=[round(x, 5) for x in (ms, a[0], a[-1])],
                   kv_tbps=round(kv_bytes / ms / 1e9, 3), tflops=round(2 * (D + DL) * B * H * Sq * L / ms / 1e9, 1),
                   hbm_bound_ms=round(kv_bytes / MLA_HBM_TBPS / 1e9, 5),
                   mfma_bound_ms=round(wave_mfmas * MLA_MFMA_CYCLES / MLA_LOADED_GHZ / 1e6 / min(MLA_CUS, plan["grid"]), 5))
        if beside_torch:
            out.update(torch_ms=[round(x, 5) for x in (statistics.median(b), b[0], b[-1])], speedup=round(statistics.median(b) / ms, 3),
                       max_diff_vs_torch=round((mla().float() - torch_ops().float()).abs().max().item(), 5))
        for page in pages:
            if L % page:
                continue
            n = L // page
            perm = torch.randperm(B * n, device=dev, generator=g)
            pool = torch.empty(B * n, page, D, device=dev, dtype=torch.bfloat16)
            pool[perm] = KV.view(B * n, page, D)
            table = perm.view(B, n).to(torch.int32)
            paged = lambda: fa.flash_attention_mla_decode_paged(Q, pool, table, lens, O=O, workspace=ws)
            w = sorted(timed(paged, args.steps, args.warmup) for _ in range(args.repeats))
            out.setdefault("paged_ms", {})[page] = [round(x, 5) for x in (statistics.median(w), w[0], w[-1])]
            out.setdefault("paged_ratio", {})[page] = round(statistics.median(w) / ms, 4)
            del pool, table
        print(json.dumps(out), flush=True)
        del Q, KV, O, ws, q2, kt, v
        torch.cuda.empty_cache()


def tree_main(args, fa, dev):
    """--tree N[,N...]: flash_attention_tree on the decode shapes with N draft nodes per sequence, beside its causal twin, alternated"""
    import torch
    f8 = torch.float8_e4m3fn
    nodes = [int(x) for x in args.tree.split(",") if x]
    pages = [int(x) for x in (args.paged or "").split(",") if x]
    W = int((args.window or "0").split(",")[0])
    shapes = SHAPES
    if args.shape:
        unknown = set(args.shape) - {x[0] for x in SHAPES + EXTRA}
        if unknown:
            raise SystemExit(f"unknown shape(s): {sorted(unknown)}")
        shapes = [x for x in SHAPES + EXTRA if x[0] in args.shape]
    primed = False
    for name, B, H, Hkv, _, Sk, d, ragged in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        lens = [1024 + (Sk - 1024) * b // (B - 1) for b in range(B)] if ragged else [Sk] * B
        K, V = (torch.randn(B, Hkv, Sk, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        sinks = (torch.linspace(-2.0, 2.0, H) + torch.log(torch.tensor(float(max(lens)))) + 0.5).to(dev)
        forms = [("bf16", False, 0)] + ([("fp8", True, 0)] if args.kv == "fp8" else [])
        for page in pages:
            if Sk % page == 0:
                forms += [(f"paged{page}", False, page)] + ([(f"paged{page}_fp8", True, page)] if args.kv == "fp8" else [])
        if args.kv == "fp8":
            def quant(Tn):
                ds = (Tn.float().abs().amax(dim=(0, 2, 3)) / 448.0).float()
                T8 = torch.empty(Tn.shape, dtype=f8, device=dev)
                for b in range(B):     # (a batch entry at a time: no fp32 copy of the whole cache)
                    T8[b] = (Tn[b].float() / ds[:, None, None]).clamp(-448, 448).to(f8)
                return T8, ds
            (K8, kds), (V8, vds) = quant(K), quant(V)
        for form, fp8, page in forms:
            Kc, Vc, table = (K8, V8, None) if fp8 else (K, V, None)
            kw = dict(k_descale=kds, v_descale=vds) if fp8 else {}
            if page:
                n = Sk // page
                perm = torch.randperm(B * n, device=dev, generator=g)
                table = perm.reshape(B, n).to(torch.int32)
                pools = []
                for Tn in (Kc, Vc):
                    Tn = Tn.view(torch.uint8) if fp8 else Tn      # (pages are moved as bytes)
                    pool = torch.empty(B * n, Hkv, page, d, device=dev, dtype=Tn.dtype)
                    pool[perm] = Tn.view(B, Hkv, n, page, d).transpose(1, 2).reshape(B * n, Hkv, page, d)
                    pools.append(pool.view(f8) if fp8 else pool)
                Kc, Vc = pools
            line = {"shape": name, "form": form, "window": W, "splits": {}, "causal_ms": {}, "tree_ms": {}, "tree_ratio": {}, "chain_equal": {}}
            for N in nodes:
                Q = torch.randn(B, H, N, d, device=dev, generator=g).to(torch.bfloat16)
                plan = fa.tree_plan(B, H, Hkv, N, Sk, d, fa.FA_DTYPE_BF16, 0, window=W)
                twin_front = getattr(fa, ("flash_attention_decode" if N <= fa.FA_DECODE_MAX_Q else "flash_attention_extend")
                                     + ("_paged" if page else "") + ("" if N <= fa.FA_DECODE_MAX_Q else "_window"))
                tree_front = fa.flash_attention_tree_paged if page else fa.flash_attention_tree
                cache = [Kc, Vc] + ([table] if page else [])
                binary = fa.tree_mask_from_parents(torch.tensor([[(i - 1) // 2 if i else -1 for i in range(N)]] * B, device=dev))
                chain = fa.tree_mask_from_parents(torch.tensor([[i - 1 for i in range(N)]] * B, device=dev))
                # (both fronts allocate O and the workspace themselves: the tree fronts take neither)
                causal = lambda: twin_front(Q, *cache, lens_d, is_causal=True, window=W, sinks=sinks, **kw)
                tree = lambda: tree_front(Q, *cache, binary, lens_d, window=W, sinks=sinks, **kw)
                # one bit-equality check per form and node count: a chain is the twin
                a = twin_front(Q, *cache, lens_d, is_causal=True, window=W, sinks=sinks, return_lse=True, **kw)
                b = tree_front(Q, *cache, chain, lens_d, window=W, sinks=sinks, return_lse=True, **kw)
                line["chain_equal"][str(N)] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
                if not primed:   # >= 1 s of calls before the first timed window
                    t = 0.0
                    while t < 1000.0:
                        t += timed(causal, 50, 0) * 50
                    primed = True
                a, b = [], []
                for _ in range(args.repeats):
                    a.append(timed(causal, args.steps, args.warmup))
                    b.append(timed(tree, args.steps, args.warmup))
                a, b = sorted(a), sorted(b)
                line["splits"][str(N)] = plan["num_splits"]
                line["causal_ms"][str(N)] = [round(x, 5) for x in (statistics.median(a), a[0], a[-1])]
                line["tree_ms"][str(N)] = [round(x, 5) for x in (statistics.median(b), b[0], b[-1])]
                line["tree_ratio"][str(N)] = round(statistics.median(b) / statistics.median(a), 4)
                del Q
            print(json.dumps(line), flush=True)
        del K, V
        if args.kv == "fp8":
            del K8, V8
        torch.cuda.empty_cache()


def accept_main(args, fa, dev):
    """--accept --tree N[,N...]: kv_cache_accept* beside the gather-and-re-append route, rope_cache_append*(pos_offsets=) beside its twin"""
    import torch
    bf, f8 = torch.bfloat16, torch.float8_e4m3fn
    nodes = [int(x) for x in args.tree.split(",") if x]
    pages = [int(x) for x in (args.paged or "").split(",") if x]
    shapes = [x for x in SHAPES + EXTRA if x[0] in args.shape] if args.shape else SHAPES
    stats = lambda v: [round(x, 5) for x in (statistics.median(v), min(v), max(v))]
    primed = False
    for name, B, H, Hkv, _, Sk, d, ragged in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        lens = [1024 + (Sk - 1024) * b // (B - 1) for b in range(B)] if ragged else [Sk] * B
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)                 # the draft counted
        table_cs = fa.rope_table(Sk, d, device=dev)
        kds, vds = (torch.rand(Hkv, device=dev, generator=g) * 0.05 + 0.01 for _ in range(2))
        forms = [("bf16", False, 0)] + ([("fp8", True, 0)] if args.kv == "fp8" else [])
        for page in pages:
            if Sk % page == 0:
                forms += [(f"paged{page}", False, page)] + ([(f"paged{page}_fp8", True, page)] if args.kv == "fp8" else [])
        for form, fp8, page in forms:
            cdt = f8 if fp8 else bf
            kw = dict(k_descale=kds, v_descale=vds) if fp8 else {}
            if page:
                n_pages = Sk // page
                table = torch.randperm(B * n_pages, device=dev, generator=g).reshape(B, n_pages).to(torch.int32)
                shape = (B * n_pages, Hkv, page, d)
            else:
                table, shape = None, (B, Hkv, Sk, d)
            tables = [table] if page else []
            Kc, Vc = (torch.zeros(shape, device=dev, dtype=torch.uint8 if fp8 else bf).view(cdt) for _ in range(2))
            p = "_paged" if page else ""
            rope_front, accept_front = getattr(fa, "rope_cache_append" + p), getattr(fa, "kv_cache_accept" + p)
            append_front, append_varlen = getattr(fa, "kv_cache_append" + p), getattr(fa, "kv_cache_append" + p + "_varlen")
            rope_varlen = getattr(fa, "rope_cache_append" + p + "_varlen")
            line = {"shape": name, "form": form, "rope": bool(args.rope), "path": {}, "accept_ms": {}, "reappend_ms": {}, "accept_ratio": {},
                    "accept_equals_reappend": {}, "rope_append_ms": {}, "rope_pos_ms": {}, "rope_pos_ratio": {}, "twin_span": {}}
            for N in nodes:
                parents = torch.tensor([[(i - 1) // 2 if i else -1 for i in range(N)]] * B, device=dev)
                depths = fa.tree_depths(parents)
                idx, nacc = fa.tree_path(parents, torch.full((B,), N - 1, device=dev))
                n = int(nacc[0])                                                   # (known from the tree's shape: read once, outside every timed call)
                Q = torch.randn(B, H, N, d, device=dev, generator=g).to(bf)
                Kn, Vn = (torch.randn(B, Hkv, N, d, device=dev, generator=g).to(bf) for _ in range(2))
                Qo = torch.empty_like(Q)
                # the draft in the caches, as the step leaves it before the acceptance
                if args.rope:
                    rope_front(Q, Kn, Vn, Kc, Vc, *tables, table_cs, lens_d, Q_out=Qo, pos_offsets=depths, **kw)
                else:
                    append_front(Kn, Vn, Kc, Vc, *tables, lens_d, **kw)
                after = lens_d - (N - nacc)                                        # the rewound lengths
                cu = (torch.arange(B + 1, device=dev) * n).to(torch.int32)
                take = idx[:, :n].long()                                           # [B, n]

                def packed(x):      # the accepted rows of [B, heads, N, d], packed by token: [B n, heads, d]
                    return torch.gather(x.transpose(1, 2), 1, take[:, :, None, None].expand(B, n, x.shape[1], d)).reshape(B * n, x.shape[1], d)

                Qa = torch.empty(B * n, H, d, device=dev, dtype=bf)

                def accept(K=Kc, V=Vc):
                    accept_front(K, V, *tables, idx, nacc, lens_d)

                def reappend(K=Kc, V=Vc):
                    if args.rope:
                        rope_varlen(packed(Q), packed(Kn), packed(Vn), K, V, *tables, cu, table_cs, after, Q_out=Qa, **kw)
                    else:
                        append_varlen(packed(Kn), packed(Vn), K, V, *tables, cu, after, **kw)

                copies = [(Kc.clone(), Vc.clone()) for _ in range(2)]
                accept(*copies[0])
                reappend(*copies[1])
                same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*copies))
                moved = not torch.equal(copies[0][0].view(torch.uint8), Kc.view(torch.uint8))
                line["accept_equals_reappend"][str(N)] = bool(same and (moved or n == N))
                del copies
                twin = lambda: rope_front(Q, Kn, Vn, Kc, Vc, *tables, table_cs, lens_d, Q_out=Qo, **kw)
                pos = lambda: rope_front(Q, Kn, Vn, Kc, Vc, *tables, table_cs, lens_d, Q_out=Qo, pos_offsets=depths, **kw)
                if not primed:   # >= 1 s of calls before the first timed window
                    t = 0.0
                    while t < 1000.0:
                        t += timed(twin, 50, 0) * 50
                    primed = True
                t = {"accept": [], "reappend": [], "twin": [], "pos": []}
                for _ in range(args.repeats):      # alternated: one window of each
                    t["twin"].append(timed(twin, args.steps, args.warmup))
                    t["pos"].append(timed(pos, args.steps, args.warmup))
                    t["accept"].append(timed(accept, args.steps, args.warmup))
                    t["reappend"].append(timed(reappend, args.steps, args.warmup))
                line["path"][str(N)] = n
                line["accept_ms"][str(N)], line["reappend_ms"][str(N)] = stats(t["accept"]), stats(t["reappend"])
                line["accept_ratio"][str(N)] = round(statistics.median(t["accept"]) / statistics.median(t["reappend"]), 4)
                line["rope_append_ms"][str(N)], line["rope_pos_ms"][str(N)] = stats(t["twin"]), stats(t["pos"])
                line["rope_pos_ratio"][str(N)] = round(statistics.median(t["pos"]) / statistics.median(t["twin"]), 4)
                line["twin_span"][str(N)] = round(max(t["twin"]) / min(t["twin"]), 4)
                del Q, Kn, Vn, Qo, Qa
            print(json.dumps(line), flush=True)
            del Kc, Vc
            torch.cuda.empty_cache()


def rope_main(args, fa, dev):
    import torch
    bf = torch.bfloat16
    shapes = [x for x in SHAPES + EXTRA if x[0] in args.shape] if args.shape else SHAPES
    for name, B, H, Hkv, Sq, Sk, d, ragged in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        lens = [1024 + (Sk - 1024) * b // (B - 1) for b in range(B)] if ragged else [Sk] * B
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        table_cs = fa.rope_table(Sk, d, device=dev)
        half = d // 2
        kds, vds = (torch.rand(Hkv, device=dev, generator=g) * 0.05 + 0.01 for _ in range(2))
        forms = [("bf16", False, 0)] + ([("fp8", True, 0)] if args.kv == "fp8" else [])
        for page in (int(x) for x in (args.paged or "").split(",") if x):
            if Sk % page == 0:
                forms += [(f"paged{page}", False, page)] + ([(f"paged{page}_fp8", True, page)] if args.kv == "fp8" else [])
        line = {"shape": name, "B": B, "H": H, "Hkv": Hkv, "Sq": Sq, "Sk": Sk, "d": d, "ragged": ragged, "rot_dim": d, "repeats": args.repeats,
                "steps": args.steps}
        out = {}

        def routes(rows, L, Kc, Vc, table, kw):
            """(fused, unfused, plain append, copy of Q, the tensors) for `rows` new rows per sequence at the lengths L (None: the capacity)"""
            Q = torch.randn(B, H, rows, d, device=dev, generator=g).to(bf)
            Kn, Vn = (torch.randn(B, Hkv, rows, d, device=dev, generator=g).to(bf) for _ in range(2))
            Qo = torch.empty_like(Q)
            ar = torch.arange(rows, device=dev)
            if table is not None:
                fused = lambda: fa.rope_cache_append_paged(Q, Kn, Vn, Kc, Vc, table, table_cs, L, Q_out=Qo, **kw)
                plain_of = lambda k: fa.kv_cache_append_paged(k, Vn, Kc, Vc, table, L, **kw)
            else:
                fused = lambda: fa.rope_cache_append(Q, Kn, Vn, Kc, Vc, table_cs, L, Q_out=Qo, **kw)
                plain_of = lambda k: fa.kv_cache_append(k, Vn, Kc, Vc, L, **kw)
            Qu = torch.empty_like(Q)

            def rotate(x, c, s):
                xf = x.float()
                x1, x2 = xf[..., :half], xf[..., half:]
                return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(bf)

            def unfused():
                length = lens_d.clamp(1, Sk) if L is not None else torch.full((B,), Sk, dtype=torch.int32, device=dev)
                pos = ((length - rows)[:, None] + ar).clamp(min=0).long()
                cs = table_cs[pos]
                c, s = cs[:, None, :, :half], cs[:, None, :, half:]
                Qu.copy_(rotate(Q, c, s))
                plain_of(rotate(Kn, c, s))

            return fused, unfused, (lambda: plain_of(Kn)), (lambda: Qo.copy_(Q)), Qo, Qu, Q, Kn

        def close(a, b, x):
            """the two routes' bf16 values (x: what was rotated) or e4m3fn codes agree as the tool's docstring says"""
            if a.element_size() == 1:
                code = lambda t: (t.view(torch.uint8) & 0x7F).int() * (1 - 2 * (t.view(torch.uint8) >> 7).int())   # sign and magnitude
                return int((code(a) - code(b)).abs().max()) <= 1
            a, b = a.float(), b.float()
            return bool(((a - b).abs() <= 2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 2.0 ** -21 * float(x.float().abs().max())).all())

        for form, fp8, page in forms:
            cdt = torch.float8_e4m3fn if fp8 else bf
            kw = dict(k_descale=kds, v_descale=vds) if fp8 else {}
            if page:
                n = Sk // page
                table = torch.randperm(B * n, device=dev, generator=g).reshape(B, n).to(torch.int32)
                Kc, Vc = (torch.zeros(B * n, Hkv, page, d, device=dev, dtype=torch.uint8 if fp8 else bf).view(cdt) for _ in range(2))
            else:
                table = None
                Kc, Vc = (torch.zeros(B, Hkv, Sk, d, device=dev, dtype=torch.uint8 if fp8 else bf).view(cdt) for _ in range(2))
            fused, unfused, plain, _, Qo, Qu, Q, Kn = routes(Sq, lens_d, Kc, Vc, table, kw)
            fused()
            keptK, keptV = Kc.clone(), Vc.clone()
            Kc.view(torch.uint8).zero_()
            Vc.view(torch.uint8).zero_()
            unfused()
            res = {"rope_matches_unfused": close(Qo, Qu, Q) and close(keptK, Kc, Kn)
                   and bool(torch.equal(keptV.view(torch.uint8), Vc.view(torch.uint8)))}
            del keptK, keptV, Q, Kn
            t = {"rope_append_ms": [], "unfused_ms": [], "append_ms": []}
            for _ in range(args.repeats):      # alternated: one window of each
                t["rope_append_ms"].append(timed(fused, args.steps, args.warmup))
                t["unfused_ms"].append(timed(unfused, args.steps, args.warmup))
                t["append_ms"].append(timed(plain, args.steps, args.warmup))
            del fused, unfused, plain, Qo, Qu
            if Sk >= 4096:
                fused, unfused, plain, copy, Qo, Qu, Q, Kn = routes(4096, None, Kc, Vc, table, kw)
                steps = max(10, args.steps // 10)
                t.update(rope_fill_ms=[], unfused_fill_ms=[], fill_ms=[], q_copy_fill_ms=[])
                for _ in range(args.repeats):
                    t["rope_fill_ms"].append(timed(fused, steps, 3))
                    t["unfused_fill_ms"].append(timed(unfused, steps, 3))
                    t["fill_ms"].append(timed(plain, steps, 3))
                    t["q_copy_fill_ms"].append(timed(copy, steps, 3))
                del fused, unfused, plain, copy, Qo, Qu, Q, Kn
            res.update({k: sorted(v) for k, v in t.items()})
            out[form] = res
            del Kc, Vc
            torch.cuda.empty_cache()
        for key in ("rope_append_ms", "unfused_ms", "append_ms", "rope_fill_ms", "unfused_fill_ms", "fill_ms", "q_copy_fill_ms"):
            have = {f: v[key] for f, v in out.items() if key in v}
            if have:
                line[key] = {f: round(statistics.median(v), 5) for f, v in have.items()}
                line[key + "_min"] = {f: round(v[0], 5) for f, v in have.items()}
                line[key + "_max"] = {f: round(v[-1], 5) for f, v in have.items()}
        line["rope_matches_unfused"] = {f: v["rope_matches_unfused"] for f, v in out.items()}
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", action="append", default=None)
    ap.add_argument("--splits", default=None, help="comma-separated forced split counts: the sweep")
    ap.add_argument("--no-cross", action="store_true")
    ap.add_argument("--paged", default=None, help="comma-separated page sizes: add paged_ms per page size to every shape's line")
    ap.add_argument("--window", default=None, help="comma-separated sliding windows: add window_ms per window to every shape's line")
    ap.add_argument("--append", action="store_true", help="add append_ms / torch_append_ms / fill_ms / fill_tbps per cache form to every shape's line")
    ap.add_argument("--extend", action="store_true", help="time flash_attention_extend on its own shapes, beside the decode-slice and prefill-pair routes")
    ap.add_argument("--varlen", action="store_true", help="time flash_attention_extend_varlen on mixed batches, beside the grouped calls of today")
    ap.add_argument("--kv", default="bf16", choices=["bf16", "fp8"], help="fp8: add fp8_ms / fp8_kv_tbps (and paged_fp8_ms) to every shape's line")
    ap.add_argument("--sinks", action="store_true", help="time every shape with and without sinks=, alternated: ms, sink_ms, sink_ratio")
    ap.add_argument("--rope", action="store_true", help="time rope_cache_append* beside the unfused torch route and the plain append, alternated")
    ap.add_argument("--tree", default=None, help="comma-separated draft-node counts: time flash_attention_tree beside its causal twin, alternated")
    ap.add_argument("--cascade", action="store_true", help="time flash_attention_cascade_decode* beside flash_attention_decode* on a shared prefix, alternated; --splits s:u,...")
    ap.add_argument("--accept", action="store_true", help="with --tree N: time kv_cache_accept* beside gather + re-append, and rope_cache_append*(pos_offsets=) beside its twin")
    ap.add_argument("--mla", action="store_true", help="time flash_attention_mla_decode* beside the same problem from torch ops, alternated; --paged, --splits")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    fa = entry.load_package()
    dev = torch.device("cuda:0")
    if args.mla:
        return mla_main(args, fa, dev)
    if args.cascade:
        return cascade_main(args, fa, dev)
    if args.accept:
        if not args.tree:
            ap.error("--accept takes the draft sizes from --tree N[,N...]")
        return accept_main(args, fa, dev)
    if args.tree:
        return tree_main(args, fa, dev)
    if args.rope:
        return rope_main(args, fa, dev)
    if args.sinks:
        return sinks_main(args, fa, dev)
    if args.extend:
        return extend_main(args, fa, dev)
    if args.varlen:
        return varlen_main(args, fa, dev)
    shapes = SHAPES
    if args.shape:
        unknown = set(args.shape) - {x[0] for x in SHAPES + EXTRA}
        if unknown:
            ap.error(f"unknown shape(s): {sorted(unknown)}")
        shapes = [x for x in SHAPES + EXTRA if x[0] in args.shape]
    primed = False
    for name, B, H, Hkv, Sq, Sk, d, ragged in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        Q = torch.randn(B, H, Sq, d, device=dev, generator=g).to(torch.bfloat16)
        K, V = (torch.randn(B, Hkv, Sk, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
        lens = [1024 + (Sk - 1024) * b // (B - 1) for b in range(B)] if ragged else [Sk] * B
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        O = torch.empty(B, H, Sq, d, device=dev, dtype=torch.bfloat16)
        kv_bytes = sum(lens) * Hkv * d * 2 * 2

        def measure(ns):
            plan = fa.decode_plan(B, H, Hkv, Sq, Sk, d, fa.FA_DTYPE_BF16, ns)
            n = fa.decode_workspace_size(B, H, Sq, d, plan["num_splits"])
            ws = torch.empty(max(n, 16), dtype=torch.uint8, device=dev)
            call = lambda: fa.flash_attention_decode(Q, K, V, lens_d, O=O, workspace=ws, num_splits=ns)
            nonlocal primed
            if not primed:   # >= 1 s of calls before the first timed window
                t = 0.0
                while t < 1000.0:
                    t += timed(call, 500, 0) * 500
                primed = True
            ms = sorted(timed(call, args.steps, args.warmup) for _ in range(args.repeats))
            return plan, ms

        def quantised(T):
            # the fp8 cache of this shape: per K/V head, descale = amax / 448 (torch's cast gives NaN beyond 448: clamp)
            ds = (T.float().abs().amax(dim=(0, 2, 3)) / 448.0).float()
            T8 = torch.empty(T.shape, dtype=torch.float8_e4m3fn, device=dev)
            for b in range(B):     # (a batch entry at a time: no fp32 copy of a 1 GB cache)
                T8[b] = (T[b].float() / ds[:, None, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
            return T8, ds

        def measure_fp8(window=0):
            plan = fa.decode_plan(B, H, Hkv, Sq, Sk, d, fa.FA_DTYPE_BF16, 0, window=window)
            ws = torch.empty(max(fa.decode_workspace_size(B, H, Sq, d, plan["num_splits"]), 16), dtype=torch.uint8, device=dev)
            kw = dict(window=window) if window else {}
            call = lambda: fa.flash_attention_decode(Q, K8, V8, lens_d, O=O, workspace=ws, k_descale=kds, v_descale=vds, **kw)
            return sorted(timed(call, args.steps, args.warmup) for _ in range(args.repeats))

        def measure_window(window):
            plan = fa.decode_plan(B, H, Hkv, Sq, Sk, d, fa.FA_DTYPE_BF16, 0, window=window)
            ws = torch.empty(max(fa.decode_workspace_size(B, H, Sq, d, plan["num_splits"]), 16), dtype=torch.uint8, device=dev)
            call = lambda: fa.flash_attention_decode(Q, K, V, lens_d, O=O, workspace=ws, window=window)
            return plan, sorted(timed(call, args.steps, args.warmup) for _ in range(args.repeats))

        def measure_paged(page, fp8=False, window=0):
            # the same data in pages: page j of sequence b is rows [j page, (j + 1) page) of every K/V head, stored wherever a
            # shuffle of all B * n page numbers puts it
            n = Sk // page
            perm = torch.randperm(B * n, device=dev, generator=g)
            table = perm.reshape(B, n).to(torch.int32)
            pools = []
            for T in ((K8, V8) if fp8 else (K, V)):
                T = T.view(torch.uint8) if fp8 else T      # (pages are moved as bytes)
                pool = torch.empty(B * n, Hkv, page, d, device=dev, dtype=T.dtype)
                pool[perm] = T.view(B, Hkv, n, page, d).transpose(1, 2).reshape(B * n, Hkv, page, d)
                pools.append(pool.view(torch.float8_e4m3fn) if fp8 else pool)
            ns = fa.decode_plan(B, H, Hkv, Sq, Sk, d, fa.FA_DTYPE_BF16, 0, window=window)["num_splits"]
            ws = torch.empty(max(fa.decode_workspace_size(B, H, Sq, d, ns), 16), dtype=torch.uint8, device=dev)
            kw = dict(k_descale=kds, v_descale=vds) if fp8 else {}
            if window:
                kw["window"] = window
            call = lambda: fa.flash_attention_decode_paged(Q, pools[0], pools[1], table, lens_d, O=O, workspace=ws, **kw)
            return sorted(timed(call, args.steps, args.warmup) for _ in range(args.repeats))

        def measure_append(fp8, page):
            # a cache of this shape and form to write into (its contents do not matter), new rows ~ N(0, 1), the shape's lengths
            cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
            kw = dict(k_descale=kds, v_descale=vds) if fp8 else {}
            if page:
                n = Sk // page
                table = torch.randperm(B * n, device=dev, generator=g).reshape(B, n).to(torch.int32)
                Kc, Vc = (torch.empty(B * n, Hkv, page, d, device=dev, dtype=cdt) for _ in range(2))
                call_of = lambda Kn, Vn, L: lambda: fa.kv_cache_append_paged(Kn, Vn, Kc, Vc, table, L, **kw)
            else:
                Kc, Vc = (torch.empty(B, Hkv, Sk, d, device=dev, dtype=cdt) for _ in range(2))
                call_of = lambda Kn, Vn, L: lambda: fa.kv_cache_append(Kn, Vn, Kc, Vc, L, **kw)
            rows = lambda n: tuple(torch.randn(B, Hkv, n, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
            Kn, Vn = rows(Sq)
            ours = sorted(timed(call_of(Kn, Vn, lens_d), args.steps, args.warmup) for _ in range(args.repeats))
            # the same with torch ops: nothing built on the host per call (every length of these shapes is >= Sq: no row is dropped)
            Ku, Vu = (Kc.view(torch.uint8), Vc.view(torch.uint8)) if fp8 else (Kc, Vc)
            ar, bi = torch.arange(Sq, device=dev), torch.arange(B, device=dev)[:, None]

            def torch_append():
                pos = ((lens_d.clamp(max=Sk) - Sq)[:, None] + ar).long()
                for new, cache, ds in ((Kn, Ku, kds if fp8 else None), (Vn, Vu, vds if fp8 else None)):
                    x = (new.float() / ds[None, :, None, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8) if fp8 else new
                    if page:
                        cache[table.gather(1, pos // page).long(), :, pos % page] = x.transpose(1, 2)
                    else:
                        cache[bi, :, pos] = x.transpose(1, 2)

            Kc.view(torch.uint8).zero_()
            Vc.view(torch.uint8).zero_()
            call_of(Kn, Vn, lens_d)()
            kept = (Kc.view(torch.uint8).clone(), Vc.view(torch.uint8).clone())
            Kc.view(torch.uint8).zero_()
            Vc.view(torch.uint8).zero_()
            theirs = sorted(timed(torch_append, args.steps, args.warmup) for _ in range(args.repeats))
            same = bool(torch.equal(kept[0], Kc.view(torch.uint8)) and torch.equal(kept[1], Vc.view(torch.uint8)))
            out = {"append_ms": ours, "torch_append_ms": theirs, "append_matches_torch": same}
            del kept
            if Sk >= 4096:
                Kf, Vf = rows(4096)
                out["fill_ms"] = sorted(timed(call_of(Kf, Vf, None), max(10, args.steps // 10), 3) for _ in range(args.repeats))
                out["fill_bytes"] = B * Hkv * 4096 * d * 2 * (2 + (1 if fp8 else 2))
            return out

        if args.splits:
            for ns in [int(x) for x in args.splits.split(",")]:
                if ns > -(-Sk // 128):
                    continue
                plan, ms = measure(ns)
                print(json.dumps({"shape": name, "forced_splits": ns, "grid": plan["grid"], "ms": round(statistics.median(ms), 5),
                                  "ms_min": round(ms[0], 5), "ms_max": round(ms[-1], 5),
                                  "kv_TBps": round(kv_bytes / statistics.median(ms) / 1e9, 3)}), flush=True)
            del Q, K, V, O
            torch.cuda.empty_cache()
            continue
        plan, ms = measure(0)
        med = statistics.median(ms)
        if args.kv == "fp8":
            (K8, kds), (V8, vds) = quantised(K), quantised(V)
        line = {"shape": name, "B": B, "H": H, "Hkv": Hkv, "Sq": Sq, "Sk": Sk, "d": d, "ragged": ragged, "io": "bfloat16",
                "ms": round(med, 5), "ms_min": round(ms[0], 5), "ms_max": round(ms[-1], 5), "repeats": args.repeats, "steps": args.steps,
                "kv_MB": round(kv_bytes / 1e6, 1), "kv_TBps": round(kv_bytes / med / 1e9, 3),
                "splits": plan["num_splits"], "row_blocks": plan["row_blocks"], "grid": plan["grid"]}
        if not args.no_cross:
            cross = lambda: fa.flash_attention(Q, K, V, O)
            steps = max(10, args.steps // 10)
            cs = sorted(timed(cross, steps, 3) for _ in range(args.repeats))
            line.update(cross_ms=round(statistics.median(cs), 5), cross_ms_min=round(cs[0], 5), cross_ms_max=round(cs[-1], 5),
                        cross_grid=fa.plan_ex(B, H, Sq, Sk, d, False, fa.FA_DTYPE_BF16, fa.FA_DTYPE_BF16, 0)[1]["grid"],
                        speedup=round(statistics.median(cs) / med, 2))
        if args.paged:
            pm = {page: measure_paged(page) for page in (int(x) for x in args.paged.split(",")) if Sk % page == 0}
            line.update(paged_ms={str(k): round(statistics.median(v), 5) for k, v in pm.items()},
                        paged_ms_min={str(k): round(v[0], 5) for k, v in pm.items()},
                        paged_ms_max={str(k): round(v[-1], 5) for k, v in pm.items()},
                        paged_ratio={str(k): round(statistics.median(v) / med, 4) for k, v in pm.items()})
        if args.kv == "fp8":
            f8 = measure_fp8()
            fmed = statistics.median(f8)
            line.update(fp8_ms=round(fmed, 5), fp8_ms_min=round(f8[0], 5), fp8_ms_max=round(f8[-1], 5), fp8_ratio=round(fmed / med, 4),
                        fp8_kv_MB=round(kv_bytes / 2 / 1e6, 1), fp8_kv_tbps=round(kv_bytes / 2 / fmed / 1e9, 3))
            if args.paged:
                pf = {page: measure_paged(page, True) for page in (int(x) for x in args.paged.split(",")) if Sk % page == 0}
                line.update(paged_fp8_ms={str(k): round(statistics.median(v), 5) for k, v in pf.items()},
                            paged_fp8_ms_min={str(k): round(v[0], 5) for k, v in pf.items()},
                            paged_fp8_ms_max={str(k): round(v[-1], 5) for k, v in pf.items()},
                            paged_fp8_ratio={str(k): round(statistics.median(v) / fmed, 4) for k, v in pf.items()})
        if args.window:
            windows = [int(x) for x in args.window.split(",")]
            pages = [page for page in (int(x) for x in (args.paged or "").split(",") if x) if Sk % page == 0]
            med_of = lambda v: round(statistics.median(v), 5)
            wbytes = {W: sum(min(L, W + Sq - 1) for L in lens) * Hkv * d * 2 * 2 for W in windows}
            wm = {W: measure_window(W) for W in windows}
            line.update(window_ms={str(W): med_of(v) for W, (_, v) in wm.items()},
                        window_ms_min={str(W): round(v[0], 5) for W, (_, v) in wm.items()},
                        window_ms_max={str(W): round(v[-1], 5) for W, (_, v) in wm.items()},
                        window_splits={str(W): pl["num_splits"] for W, (pl, _) in wm.items()},
                        window_kv_MB={str(W): round(wbytes[W] / 1e6, 2) for W in windows},
                        window_kv_tbps={str(W): round(wbytes[W] / statistics.median(v) / 1e9, 3) for W, (_, v) in wm.items()})
            if pages:
                line.update(window_paged_ms={str(page): {str(W): med_of(measure_paged(page, False, W)) for W in windows} for page in pages})
            if args.kv == "fp8":
                wf = {W: measure_fp8(W) for W in windows}
                line.update(window_fp8_ms={str(W): med_of(v) for W, v in wf.items()},
                            window_fp8_kv_tbps={str(W): round(wbytes[W] / 2 / statistics.median(v) / 1e9, 3) for W, v in wf.items()})
                if pages:
                    line.update(window_paged_fp8_ms={str(page): {str(W): med_of(measure_paged(page, True, W)) for W in windows}
                                                     for page in pages})
        if args.append:
            forms = [("bf16", False, 0)] + ([("fp8", True, 0)] if args.kv == "fp8" else [])
            for page in (int(x) for x in (args.paged or "").split(",") if x):
                if Sk % page == 0:
                    forms += [(f"paged{page}", False, page)] + ([(f"paged{page}_fp8", True, page)] if args.kv == "fp8" else [])
            am = {form: measure_append(fp8, page) for form, fp8, page in forms}
            for key in ("append_ms", "torch_append_ms", "fill_ms"):
                have = {f: v[key] for f, v in am.items() if key in v}
                line[key] = {f: round(statistics.median(v), 5) for f, v in have.items()}
                line[key + "_min"] = {f: round(v[0], 5) for f, v in have.items()}
                line[key + "_max"] = {f: round(v[-1], 5) for f, v in have.items()}
            line["append_matches_torch"] = {f: v["append_matches_torch"] for f, v in am.items()}
            line["fill_tbps"] = {f: round(v["fill_bytes"] / statistics.median(v["fill_ms"]) / 1e9, 3) for f, v in am.items() if "fill_ms" in v}
        if args.kv == "fp8":
            del K8, V8
        print(json.dumps(line), flush=True)
        del Q, K, V, O
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
