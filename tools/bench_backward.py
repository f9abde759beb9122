#!/usr/bin/env python3
"""Time flash_attention_backward: one JSON line per shape.

  python3 tools/bench_backward.py [--steps N] [--warmup W]

Shapes: B 8 H 16 S 4096 d 128 without and with the causal mask, and the anchor shape B 16 H 16 S 2048 d 128 (bf16 I/O).  Each line:
  ms                 one backward call (its three kernels and the Python binding), hipEvents around --steps calls after --warmup
                     calls of the same shape; the device is primed first with >= 1 s of backward calls
  tflops             10 B H Sq Sk d FLOPs per backward (half of it under the causal mask with Sq = Sk) / ms
  dq_atomic_TBps     dQ's fp32 atomic bytes (4 B H Sq d per 256-key block) / ms: against the ~1.3 TB/s chip-wide atomic rate
  fwd_ms, fwd_tflops the forward on the same tensors (4 B H Sq Sk d, halved under the mask)
  sdpa_bwd_ms        torch's scaled_dot_product_attention backward on the same tensors, when it runs (not a gate)
Times per kernel (pre-pass, main kernel, post-pass) are not taken here: they come from a run of this script under
`rocprofv3 --kernel-trace --stats` of its own (profiles/r05_backward_kernel_stats.csv).
--shape NAME (repeatable) runs only the named shapes.

Grouped-query shapes run only when named: gqa_B8H16kv4S4096d128_nc, gqa_B8H16kv4S4096d128_c, gqa_B8H16kv1S4096d128_nc,
gqa_B8H16kv1S4096d128_c (B 8, 16 query heads, 4 or 1 K/V heads, S 4096, d 128, fp32 O / dO / gradients).  Their lines carry, beside
the fields above for the grouped-query calls (ms, fwd_ms; FLOPs and atomic bytes are those of the 16 query heads):
  expand_ms          K and V expanded to 16 heads with repeat_interleave: what a caller without grouped-query support does first
  mha_fwd_ms         the forward on the expanded K, V (the expansion not included)
  mha_bwd_ms         the backward on the expanded K, V: dK, dV come back per query head
  group_sum_ms       ... and are summed over each group with torch
  workaround_bwd_ms  mha backward + group sum in one timed window: the only route to dK, dV without grouped-query support
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def gqa_line(fa, torch, dev, args, name, B, H, Hkv, S, d, causal, odt, primed):
    """one grouped-query shape: the grouped calls, and the expand / MHA / group-sum workaround on the same problem"""
    G = H // Hkv
    g = torch.Generator(device=dev).manual_seed(0)
    Q, dO = (torch.randn(B, H, S, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
    K, V = (torch.randn(B, Hkv, S, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
    dOo = dO.to(odt)
    O, lse = fa.flash_attention(Q, K, V, is_causal=causal, out_dtype=odt, return_lse=True)
    dQ = torch.empty(B, H, S, d, device=dev, dtype=odt)
    dK, dV = (torch.empty(B, Hkv, S, d, device=dev, dtype=odt) for _ in range(2))
    bwd = lambda: fa.flash_attention_backward(Q, K, V, O, dOo, lse, is_causal=causal, dQ=dQ, dK=dK, dV=dV)
    if not primed:
        for _ in range(4):
            timed(bwd, 50, 0)
    t = lambda fn: round(timed(fn, args.steps, args.warmup), 4)
    ms, fwd_ms = t(bwd), t(lambda: fa.flash_attention(Q, K, V, O, is_causal=causal))
    expand = lambda: (K.repeat_interleave(G, 1), V.repeat_interleave(G, 1))
    Ke, Ve = expand()
    Oe, lsee = fa.flash_attention(Q, Ke, Ve, is_causal=causal, out_dtype=odt, return_lse=True)
    dKe, dVe = (torch.empty(B, H, S, d, device=dev, dtype=odt) for _ in range(2))
    mha = lambda: fa.flash_attention_backward(Q, Ke, Ve, Oe, dOo, lsee, is_causal=causal, dQ=dQ, dK=dKe, dV=dVe)
    gsum = lambda: (dKe.view(B, Hkv, G, S, d).sum(2), dVe.view(B, Hkv, G, S, d).sum(2))
    half = 0.5 if causal else 1.0
    flops = 10 * B * H * S * S * d * half
    line = {"shape": name, "B": B, "H": H, "Hkv": Hkv, "S": S, "d": d, "causal": causal, "io": str(odt).replace("torch.", ""),
            "ms": ms, "tflops": round(flops / ms / 1e9, 1), "main_kernel_workgroups": B * Hkv * -(-S // 256),
            "fwd_ms": fwd_ms, "fwd_tflops": round(0.4 * flops / fwd_ms / 1e9, 1),
            "expand_ms": t(expand), "mha_fwd_ms": t(lambda: fa.flash_attention(Q, Ke, Ve, Oe, is_causal=causal)),
            "mha_bwd_ms": t(mha), "group_sum_ms": t(gsum), "workaround_bwd_ms": t(lambda: (mha(), gsum()))}
    line["bwd_speedup_vs_workaround"] = round(line["workaround_bwd_ms"] / ms, 3)
    line["bwd_vs_mha_same_flops"] = round(line["mha_bwd_ms"] / ms, 3)
    line["fwd_vs_mha_expanded"] = round(line["mha_fwd_ms"] / fwd_ms, 3)
    print(json.dumps(line), flush=True)
    torch.cuda.empty_cache()
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shape", action="append", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    fa = entry.load_package()
    dev = torch.device("cuda:0")
    shapes = [("B8H16S4096d128_nc", 8, 16, 4096, 128, False, torch.float32),
              ("B8H16S4096d128_c", 8, 16, 4096, 128, True, torch.float32),
              ("anchor_B16H16S2048d128_bf16io", 16, 16, 2048, 128, False, torch.bfloat16)]
    gqa_shapes = [(f"gqa_B8H16kv{kv}S4096d128_{'c' if c else 'nc'}", 8, 16, 4096, 128, c, torch.float32, kv) for kv in (4, 1) for c in (False, True)]
    if args.shape:
        unknown = set(args.shape) - {x[0] for x in shapes + gqa_shapes}
        if unknown:
            ap.error(f"unknown shape(s): {sorted(unknown)}")
        shapes = [x for x in shapes + gqa_shapes if x[0] in args.shape]
    primed = False
    for name, B, H, S, d, causal, odt, *kv in shapes:
        if kv:
            primed = gqa_line(fa, torch, dev, args, name, B, H, kv[0], S, d, causal, odt, primed)
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        Q, K, V, dO = (torch.randn(B, H, S, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(4))
        O, lse = fa.flash_attention(Q, K, V, is_causal=causal, out_dtype=odt, return_lse=True)
        dOo = dO.to(odt)
        dQ, dK, dV = (torch.empty(B, H, S, d, device=dev, dtype=odt) for _ in range(3))
        bwd = lambda: fa.flash_attention_backward(Q, K, V, O, dOo, lse, is_causal=causal, dQ=dQ, dK=dK, dV=dV)
        if not primed:   # prime the device: >= 1 s of backward calls (~160 calls of 3.5-6.5 ms) before the first timed window
            for _ in range(4):
                timed(bwd, 50, 0)
            primed = True
        ms = timed(bwd, args.steps, args.warmup)
        fwd_ms = timed(lambda: fa.flash_attention(Q, K, V, O, is_causal=causal), args.steps, args.warmup)
        half = 0.5 if causal else 1.0
        flops = 10 * B * H * S * S * d * half
        n_blocks = -(-S // 256)
        atomic_bytes = 4 * B * H * S * d * (n_blocks if not causal else (n_blocks + 1) / 2)
        line = {"shape": name, "B": B, "H": H, "S": S, "d": d, "causal": causal, "io": str(odt).replace("torch.", ""),
                "ms": round(ms, 4), "tflops": round(flops / ms / 1e9, 1),
                "dq_atomic_bytes": int(atomic_bytes), "dq_atomic_TBps": round(atomic_bytes / ms / 1e9, 3),
                "fwd_ms": round(fwd_ms, 4), "fwd_tflops": round(0.4 * flops / fwd_ms / 1e9, 1)}
        try:
            q, k, v = (t.clone().requires_grad_() for t in (Q, K, V))
            o = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal)
            line["sdpa_bwd_ms"] = round(timed(lambda: torch.autograd.grad(o, (q, k, v), dO, retain_graph=True), args.steps,
                                              args.warmup), 4)
        except Exception as e:  # noqa: BLE001 -- reported, not a gate
            line["sdpa_bwd_ms"] = None
            line["sdpa_error"] = f"{type(e).__name__}: {str(e)[:120]}"
        print(json.dumps(line), flush=True)
        del Q, K, V, dO, O, lse, dOo, dQ, dK, dV
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
