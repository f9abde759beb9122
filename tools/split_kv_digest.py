#!/usr/bin/env python3
"""Digests of what the split-KV kernel computes: one line per case with a SHA-256 of the bytes of every O and LSE of the case.

  python3 tools/split_kv_digest.py > split_kv_digest.log

For a change of decode_bf16.hip.h that is meant to leave every result bit as it is: run at both commits and compare the two logs
line for line (profiles/split_kv_digest_parent.log, profiles/split_kv_digest.log).  Inputs are built on the CPU from fixed seeds, so a
line depends on the library alone.

Every case: B = 2, Hkv = 2, capacity 384 (three 128-key tiles).  A case is one line, the product of
  call     decode, extend
  d        64, 128
  G        1, 4 query heads per K/V head
  Sq       decode 1, 5, 16; extend 5, 17, 40, 130 (a row block of 32 or 64 packed rows ends inside a head, at a head boundary and
           past the last row)
  causal   0, 1
  splits   forced 1, 3
  window   decode 0, 7, 130 (130 under length 300: the first tile is not the sequence's tile 0); extend has none
  kv       bf16, fp8 (e4m3fn with descales 0.75, 1.5 for K and 1.25, 0.5 for V)
and its digest is fed, in this order, by the 24 calls of
  cache    contig, paged16, paged128 (shuffled block table), each also as a strided view ([.., rows, Hkv, d] storage)
  out      f32, bf16
  lengths  (1, 300), (129, 300)
so that the log stays small enough to commit (416 lines); a line that differs names the case to take apart.

After those, in a second pass over d (so that the lines above keep their content and order):
  extend   with window 7, 130: the cases above with the windowed call (flash_attention_extend*_window(window=W)), 256 lines
  varlen   the ragged call on token-packed Q, both sequences with rows of their own -- rows (5, 130) and (17, 40) -- G, causal,
           splits, kv as above, window 0, 7, 130; the same 24 calls per line, 192 lines

After those 864 lines, in a third pass (so that they keep their content and order): every case above once more, in the same order, as
the call WITH attention sinks (``sinks=``: the flash_attention_sink_* entry points), each line prefixed "sink" and carrying the first 16
hex digits of its SHA-256 (profiles/sink_digest.log holds these lines alone): 864 lines more.  The
sink vector at H = 8 is (-inf, 0, 1.5, 3, 4.5, 5.5, 6.5, 8); at H = 2 it is (0, 5.5), every fourth element from the second
(tests/sink_check.py: sinks_for).
"""
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, HKV, CAP = 2, 2, 384
LENS = [(1, 300), (129, 300)]
SINKS8 = (float("-inf"), 0.0, 1.5, 3.0, 4.5, 5.5, 6.5, 8.0)


def main():
    import torch
    import __graft_entry__ as entry
    fa = entry.load_package()
    dev = torch.device("cuda:0")
    f8 = torch.float8_e4m3fn
    lens_d = [torch.tensor(v, dtype=torch.int32).to(dev) for v in LENS]
    kds, vds = torch.tensor([0.75, 1.5]), torch.tensor([1.25, 0.5])

    def caches_of(d):
        g = torch.Generator().manual_seed(1000 + d)
        K, V = (torch.randn(B, HKV, CAP, d, generator=g).to(torch.bfloat16) for _ in range(2))
        # the cache forms of this d: name -> (K, V, block table or None, descales or None), all on the device
        caches = {}
        for kv in ("bf16", "fp8"):
            if kv == "fp8":
                Kc, Vc = ((T.float() / ds[None, :, None, None]).clamp(-448, 448).to(f8) for T, ds in ((K, kds), (V, vds)))
                desc = dict(k_descale=kds.to(dev), v_descale=vds.to(dev))
            else:
                Kc, Vc, desc = K, V, {}
            strided = lambda T: T.transpose(1, 2).contiguous().to(dev).transpose(1, 2)   # [.., rows, Hkv, d] storage
            caches["contig", kv] = (Kc.to(dev), Vc.to(dev), None, desc)
            caches["contig+s", kv] = (strided(Kc), strided(Vc), None, desc)
            for page in (16, 128):
                n = CAP // page
                perm = torch.randperm(B * n + 3, generator=torch.Generator().manual_seed(page))[:B * n]
                pools = []
                for T in (Kc, Vc):
                    pool = torch.zeros(B * n + 3, HKV, page, d, dtype=torch.uint8 if kv == "fp8" else T.dtype)
                    pool[perm] = (T.view(torch.uint8) if kv == "fp8" else T).view(B, HKV, n, page, d).transpose(1, 2).reshape(B * n, HKV, page, d)
                    pools.append(pool.view(f8) if kv == "fp8" else pool)
                table = perm.reshape(B, n).to(torch.int32).to(dev)
                caches[f"paged{page}", kv] = (pools[0].to(dev), pools[1].to(dev), table, desc)
                caches[f"paged{page}+s", kv] = (strided(pools[0]), strided(pools[1]), table, desc)
        return caches

    def sinks_of(H, on):
        """the keyword of the third pass: the sink vector of H query heads"""
        if not on:
            return {}
        step = max(len(SINKS8) // H, 1)
        return dict(sinks=torch.tensor([SINKS8[(1 + h * step) % len(SINKS8)] if H < len(SINKS8) else SINKS8[h % len(SINKS8)]
                                        for h in range(H)], dtype=torch.float32).to(dev))

    def uniform(d, caches, cases, sinks=False):
        for call, sqs, windows in cases:
            for G, Sq in itertools.product((1, 4), sqs):
                gq = torch.Generator().manual_seed(7 * d + 1000 * G + Sq)
                Q = torch.randn(B, HKV * G, Sq, d, generator=gq).to(torch.bfloat16).to(dev)
                for causal, ns, W, kv in itertools.product((0, 1), (1, 3), windows, ("bf16", "fp8")):
                    h = hashlib.sha256()
                    for form, out, L in itertools.product([f for f, k in caches if k == kv], (torch.float32, torch.bfloat16), lens_d):
                        Kc, Vc, table, desc = caches[form, kv]
                        kw = dict(desc, is_causal=bool(causal), num_splits=ns, return_lse=True, out_dtype=out, **sinks_of(HKV * G, sinks))
                        if call == "decode" or W:
                            kw["window"] = W
                        win = "_window" if call == "extend" and W else ""     # (the extend fronts take a window under a name of their own)
                        if table is None:
                            O, lse = getattr(fa, f"flash_attention_{call}{win}")(Q, Kc, Vc, L, **kw)
                        else:
                            O, lse = getattr(fa, f"flash_attention_{call}_paged{win}")(Q, Kc, Vc, table, L, **kw)
                        h.update(O.cpu().view(torch.uint8).numpy().tobytes())
                        h.update(lse.cpu().numpy().tobytes())
                    print(f"{'sink ' if sinks else ''}{call} d{d} G{G} Sq{Sq} causal{causal} splits{ns} window{W} {kv} {h.hexdigest()[:16 if sinks else 64]}")

    def ragged(d, caches, sinks=False):
        for G, sq in itertools.product((1, 4), ((5, 130), (17, 40))):
            gq = torch.Generator().manual_seed(7 * d + 1000 * G + sum(sq))
            Q = torch.randn(sum(sq), HKV * G, d, generator=gq).to(torch.bfloat16).to(dev)
            cu = torch.tensor([0, sq[0], sum(sq)], dtype=torch.int32).to(dev)
            for causal, ns, W, kv in itertools.product((0, 1), (1, 3), (0, 7, 130), ("bf16", "fp8")):
                h = hashlib.sha256()
                for form, out, L in itertools.product([f for f, k in caches if k == kv], (torch.float32, torch.bfloat16), lens_d):
                    Kc, Vc, table, desc = caches[form, kv]
                    kw = dict(desc, is_causal=bool(causal), num_splits=ns, return_lse=True, out_dtype=out, **(dict(window=W) if W else {}),
                              **sinks_of(HKV * G, sinks))
                    if table is None:
                        O, lse = (fa.flash_attention_extend_varlen_window if W else fa.flash_attention_extend_varlen)(Q, Kc, Vc, cu, L, **kw)
                    else:
                        O, lse = (fa.flash_attention_extend_paged_varlen_window if W else fa.flash_attention_extend_paged_varlen)(
                            Q, Kc, Vc, table, cu, L, **kw)
                    h.update(O.cpu().view(torch.uint8).numpy().tobytes())
                    h.update(lse.cpu().numpy().tobytes())
                print(f"{'sink ' if sinks else ''}varlen d{d} G{G} rows{sq[0]}+{sq[1]} causal{causal} splits{ns} window{W} {kv} "
                      f"{h.hexdigest()[:16 if sinks else 64]}")

    for d in (64, 128):
        uniform(d, caches_of(d), (("decode", (1, 5, 16), (0, 7, 130)), ("extend", (5, 17, 40, 130), (0,))))
    for d in (64, 128):
        caches = caches_of(d)
        uniform(d, caches, (("extend", (5, 17, 40, 130), (7, 130)),))
        ragged(d, caches)
    for d in (64, 128):
        uniform(d, caches_of(d), (("decode", (1, 5, 16), (0, 7, 130)), ("extend", (5, 17, 40, 130), (0,))), sinks=True)
    for d in (64, 128):
        caches = caches_of(d)
        uniform(d, caches, (("extend", (5, 17, 40, 130), (7, 130)),), sinks=True)
        ragged(d, caches, sinks=True)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
