"""The fixed adversarial cases of the backward pass: data off the N(0,1) / scale = 1/sqrt(d) path.  tests/test_backward_edges.py
runs them on the GPU, tests/test_grad_check.py runs the checker's emulation and wrong-answer controls on them on the CPU.

  scale    a scale other than 1/sqrt(d): 0.02, 3/sqrt(d), and 1 with Q and K scaled by d^-1/4 so the scores stay O(1)
  sharp    Q and K times 3 and times 12 (the `boost` of tests/fuzz_gpu.py; at 12 the LSE reaches hundreds and the forward's optimistic
           pass falls back), on every (O / dO, gradient) type pair
  offset   Q with mean 2 in every coordinate and K with a constant 8 along that direction: a common score offset of 16 d scale, so the
           LSE is large and every S - LSE a difference of large numbers
  large    V and dO times 2^13 and times 2^-13
  onehot   every query row matches one key: P is one-hot to fp32, dQ and dK are zero in exact arithmetic, dV a scatter of dO
"""
import collections
import functools

import torch

import grad_check as gc

Case = collections.namedtuple("Case", "name d Sq Sk H Hkv causal kind param o_dtype grad_dtype")

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)]     # as tests/test_backward.py
MHA, G4, MQA = (2, 2), (8, 2), (4, 1)                             # (H, Hkv)
_short = {F32: "f32", BF16: "bf16"}


def _cases():
    out = []

    def add(kind, param, d, shape, heads, causal, dt):
        name = f"{kind}{param}-d{d}-{shape[0]}x{shape[1]}-H{heads[0]}kv{heads[1]}-{'causal' if causal else 'full'}-{_short[dt[0]]}-{_short[dt[1]]}"
        out.append(Case(name, d, shape[0], shape[1], heads[0], heads[1], causal, kind, param, dt[0], dt[1]))

    add("scale", "small", 64, (320, 320), MHA, True, DTYPES[0])
    add("scale", "small", 128, (128, 700), G4, False, DTYPES[1])
    add("scale", "large", 128, (1000, 1000), G4, True, DTYPES[2])
    add("scale", "large", 64, (700, 128), MHA, False, DTYPES[3])
    add("scale", "one", 64, (1000, 1000), MQA, False, DTYPES[0])
    add("scale", "one", 128, (320, 320), MHA, True, DTYPES[3])
    sharp = [(3, 64, False, (320, 320), G4), (3, 64, True, (1000, 1000), MHA), (3, 128, False, (128, 700), MQA),
             (3, 128, True, (700, 128), G4), (12, 64, False, (700, 128), MQA), (12, 64, True, (2048, 2048), MHA),
             (12, 128, False, (1000, 1000), G4), (12, 128, True, (2048, 2048), MQA)]
    for boost, d, causal, shape, heads in sharp:
        for dt in DTYPES:
            add("sharp", boost, d, shape, heads, causal, dt)
    add("offset", "", 64, (1000, 1000), MHA, True, DTYPES[0])
    add("offset", "", 128, (320, 320), G4, False, DTYPES[3])
    add("large", 13, 128, (320, 320), G4, True, DTYPES[0])
    add("large", -13, 64, (128, 700), MHA, False, DTYPES[3])
    add("onehot", "", 64, (320, 320), MHA, True, DTYPES[0])
    add("onehot", "", 128, (700, 128), G4, False, DTYPES[0])
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def scale_of(c):
    if c.kind == "scale":
        return {"small": 0.02, "large": 3.0 / c.d ** 0.5, "one": 1.0}[c.param]
    return 1.0 / c.d ** 0.5


def hot_key(q, Sk, causal):
    """the key row q of a onehot case matches (visible under the mask)"""
    return (7 * q + 3) % (min(q + 1, Sk) if causal else Sk)


def _data_key(c):
    return c[1:9]          # everything but the name and the output types


@functools.lru_cache(maxsize=2)
def _data(key):
    d, Sq, Sk, H, Hkv, causal, kind, param = key
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in f"{kind}{param}") * 1000 + d + Sq + 3 * Sk + 7 * H + causal)
    rn = lambda *shape: torch.randn(shape, generator=g)
    Q, K, V, dO = rn(1, H, Sq, d), rn(1, Hkv, Sk, d), rn(1, Hkv, Sk, d), rn(1, H, Sq, d)
    if kind == "scale" and param == "one":
        Q, K = Q * d ** -0.25, K * d ** -0.25
    elif kind == "sharp":
        Q, K = Q * param, K * param
    elif kind == "offset":
        Q, K = Q + 2.0, K + 8.0
    elif kind == "large":
        V, dO = V * 2.0 ** param, dO * 2.0 ** param
    elif kind == "onehot":
        K = torch.where(K > 0, 1.0, -1.0)
        keys = torch.tensor([hot_key(q, Sk, causal) for q in range(Sq)])
        Q = 16.0 * K[:, :, keys].repeat_interleave(H // Hkv, dim=1)
    return tuple(t.bfloat16() for t in (Q, K, V, dO))


def build(c):
    """bf16 CPU tensors Q [1, H, Sq, d], K, V [1, Hkv, Sk, d], dO (bf16-valued, to be passed in c.o_dtype), and the scale"""
    return (*_data(_data_key(c)), scale_of(c))


@functools.lru_cache(maxsize=2)
def _truth(key, scale):
    Q, K, V, dO = _data(key)
    causal = key[5]
    return gc.reference_grads(Q, K, V, scale, causal, dO=dO)[0], gc.magnitudes(Q, K, V, dO, scale, causal)


def truth(c):
    """(float64 reference gradients, magnitudes) of the case; cached across the type pairs of the same data"""
    return _truth(_data_key(c), scale_of(c))
