#!/usr/bin/env python3
"""Time flash_attention_mla_prefill (bf16 in and out, 192 score / 128 value columns) against the routes a caller has without it: one JSON
line per shape.  Needs a GPU.

  python3 tools/bench_mla_prefill.py [--window SECONDS] [--shape NAME ...]

Shapes (B, H, Sq = Sk): B1H128S4096_c, B1H128S8192_c, B4H16S4096_c, B8H16S2048_c (causal) and B1H128Sq2048Sk8192_nc.  Every route of a
shape is warmed, then timed in windows of at least --window seconds (default 0.3; hipEvents around as many calls as fill it), five
rounds with the routes ALTERNATING inside a round; a figure is the median of its five windows, `spread` the largest
(max - min) / median of any route of the line.  Routes:
  mla_prefill_ms     the call through the Python front, default flags; tflops counts 192 + 128 multiply-adds per visible (row, key) pair
  single_weights_ms  the same with FA_FLAG_BF16_WEIGHTS: what the bf16 hi + lo pair costs on the early rows is the difference
  padded_ms          the route without this call: flash_attention at d = 192 on V zero-padded to 192 columns (the padding itself not
                     timed).  It is run on `padded_heads` of the B * H heads -- what takes about a window -- and the figure is that
                     time scaled LINEARLY to all heads (one workgroup per head and query block: the kernel's time is linear in heads)
  torch_ms           bf16 matmul, fp32 softmax, bf16 matmul, over the heads in chunks whose score matrix holds at most 2^29 elements
  d128_ms            this library's flash_attention at d = 128 on the same B, H, S and mask: the nearest tuned kernel; `vs_d128` is
                     mla_prefill_ms / d128_ms, to be read beside the multiply-add ratio 320 / 256 = 1.25
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("B1H128S4096_c", 1, 128, 4096, 4096, True), ("B1H128S8192_c", 1, 128, 8192, 8192, True), ("B4H16S4096_c", 4, 16, 4096, 4096, True),
          ("B8H16S2048_c", 8, 16, 2048, 2048, True), ("B1H128Sq2048Sk8192_nc", 1, 128, 2048, 8192, False)]
TORCH_MAX_SCORES = 1 << 29   # elements of the score matrix the torch route materialises at a time: it walks the heads in such chunks


def window(torch, fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--shape", action="append", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mla_prefill: needs a GPU")
    import __graft_entry__ as entry
    fa = entry.load_package()
    dev, bf16 = torch.device("cuda:0"), torch.bfloat16
    for name, B, H, Sq, Sk, causal in SHAPES:
        if args.shape and name not in args.shape:
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        Q = torch.randn(B, H, Sq, 192, device=dev, generator=g).to(bf16)
        K = torch.randn(B, H, Sk, 192, device=dev, generator=g).to(bf16)
        V = torch.randn(B, H, Sk, 128, device=dev, generator=g).to(bf16)
        O = torch.empty(B, H, Sq, 128, device=dev, dtype=bf16)
        scale = 192 ** -0.5
        routes = {"mla_prefill_ms": lambda: fa.flash_attention_mla_prefill(Q, K, V, O, is_causal=causal),
                  "single_weights_ms": lambda: fa.flash_attention_mla_prefill(Q, K, V, O, is_causal=causal, weights_dtype=bf16)}
        Q1, K1, O1 = Q[..., :128].contiguous(), K[..., :128].contiguous(), torch.empty_like(O)
        routes["d128_ms"] = lambda: fa.flash_attention(Q1, K1, V, O1, is_causal=causal)
        # the padded route on as many heads (of batch 0 .. ) as take about a window
        Qf, Kf = Q.reshape(1, B * H, Sq, 192), K.reshape(1, B * H, Sk, 192)
        Vf = torch.nn.functional.pad(V, (0, 64)).reshape(1, B * H, Sk, 192)
        padded = lambda n: fa.flash_attention(Qf[:, :n], Kf[:, :n], Vf[:, :n], is_causal=causal)
        padded(1)
        torch.cuda.synchronize()
        heads = max(1, min(B * H, int(args.window * 1e3 / window(torch, lambda: padded(1), 1))))
        routes["padded_ms"] = lambda: padded(heads)
        hidden = torch.ones(Sq, Sk, device=dev, dtype=torch.bool).triu_(1) if causal else None
        hc = max(1, TORCH_MAX_SCORES // (Sq * Sk))

        def torch_route():
            for h0 in range(0, B * H, hc):
                s = torch.matmul(Qf[0, h0:h0 + hc], Kf[0, h0:h0 + hc].transpose(-1, -2)).float().mul_(scale)
                if hidden is not None:
                    s.masked_fill_(hidden, float("-inf"))
                torch.matmul(torch.softmax(s, dim=-1).to(bf16), V.reshape(B * H, Sk, 128)[h0:h0 + hc], out=Ot[h0:h0 + hc])
        Ot = torch.empty(B * H, Sq, 128, device=dev, dtype=bf16)
        routes["torch_ms"] = torch_route
        steps = {}
        for k, fn in routes.items():   # warm, then size the window
            fn()
            torch.cuda.synchronize()
            steps[k] = max(1, math.ceil(args.window * 1e3 / window(torch, fn, 1)))
        wins = {k: [] for k in routes}
        for _ in range(5):
            for k, fn in routes.items():
                wins[k].append(window(torch, fn, steps[k]))
        med = {k: statistics.median(v) for k, v in wins.items()}
        pairs = (Sq * (Sq + 1) // 2 if causal else Sq * Sk) * B * H
        line = {"shape": name, "B": B, "H": H, "Sq": Sq, "Sk": Sk, "causal": causal}
        line.update({k: round(v, 4) for k, v in med.items()})
        line["padded_heads"] = heads
        line["padded_ms"] = round(med["padded_ms"] * B * H / heads, 2)
        line["tflops"] = round(2 * 320 * pairs / med["mla_prefill_ms"] / 1e9, 1)
        line["vs_d128"] = round(med["mla_prefill_ms"] / med["d128_ms"], 3)
        line["pair_cost"] = round(med["mla_prefill_ms"] / med["single_weights_ms"] - 1, 4)
        line["spread"] = round(max((max(v) - min(v)) / med[k] for k, v in wins.items()), 4)
        print(json.dumps(line), flush=True)
        del routes, Q, K, V, O, Qf, Kf, Vf, Ot, Q1, K1, O1
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
