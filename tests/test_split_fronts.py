"""Which C entry point every Python front of the K/V-cache calls reaches: the ten attention fronts (flash_attention_decode*,
flash_attention_extend*) between them reach the fourteen split-KV entry points of include/flash_attention.h, the four kv_cache_append*
fronts the four append entry points, and which one a call takes depends on the cache type and the window.  ``fa.lib`` is replaced by a
proxy that records the names fetched from the real library; every call's record is compared with a literal table, and every O and LSE
must be finite.  Results are checked elsewhere (test_decode*.py, test_extend*.py, test_kv_append*.py): this pins the mapping."""
import functools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, H, HKV, D, CAPACITY, PAGE = 2, 4, 2, 64, 256, 16
LENS = (200, 256)
SQ_DECODE, SQ_EXTEND, ROWS = 3, 20, (3, 20)
WINDOW = 40
WS = "flash_attention_decode_workspace_size"

# (front, fp8 cache, window) -> (the plan entry point, the launch entry point); a front without a window argument has None only
ATTENTION = {
    ("flash_attention_decode", False, None): ("flash_attention_decode_plan", "flash_attention_decode"),
    ("flash_attention_decode", True, None): ("flash_attention_decode_plan", "flash_attention_decode_fp8"),
    ("flash_attention_decode", False, WINDOW): ("flash_attention_decode_plan_window", "flash_attention_decode_window"),
    ("flash_attention_decode", True, WINDOW): ("flash_attention_decode_plan_window", "flash_attention_decode_window"),
    ("flash_attention_decode_paged", False, None): ("flash_attention_decode_plan", "flash_attention_decode_paged"),
    ("flash_attention_decode_paged", True, None): ("flash_attention_decode_plan", "flash_attention_decode_paged_fp8"),
    ("flash_attention_decode_paged", False, WINDOW): ("flash_attention_decode_plan_window", "flash_attention_decode_paged_window"),
    ("flash_attention_decode_paged", True, WINDOW): ("flash_attention_decode_plan_window", "flash_attention_decode_paged_window"),
    ("flash_attention_extend", False, None): ("flash_attention_extend_plan", "flash_attention_extend"),
    ("flash_attention_extend", True, None): ("flash_attention_extend_plan", "flash_attention_extend"),
    ("flash_attention_extend_window", False, None): ("flash_attention_extend_plan", "flash_attention_extend"),
    ("flash_attention_extend_window", True, None): ("flash_attention_extend_plan", "flash_attention_extend"),
    ("flash_attention_extend_window", False, WINDOW): ("flash_attention_extend_plan_window", "flash_attention_extend_window"),
    ("flash_attention_extend_window", True, WINDOW): ("flash_attention_extend_plan_window", "flash_attention_extend_window"),
    ("flash_attention_extend_paged", False, None): ("flash_attention_extend_plan", "flash_attention_extend_paged"),
    ("flash_attention_extend_paged", True, None): ("flash_attention_extend_plan", "flash_attention_extend_paged"),
    ("flash_attention_extend_paged_window", False, None): ("flash_attention_extend_plan", "flash_attention_extend_paged"),
    ("flash_attention_extend_paged_window", True, None): ("flash_attention_extend_plan", "flash_attention_extend_paged"),
    ("flash_attention_extend_paged_window", False, WINDOW): ("flash_attention_extend_plan_window", "flash_attention_extend_paged_window"),
    ("flash_attention_extend_paged_window", True, WINDOW): ("flash_attention_extend_plan_window", "flash_attention_extend_paged_window"),
    ("flash_attention_extend_varlen", False, None): ("flash_attention_extend_varlen_plan", "flash_attention_extend_varlen"),
    ("flash_attention_extend_varlen", True, None): ("flash_attention_extend_varlen_plan", "flash_attention_extend_varlen"),
    ("flash_attention_extend_varlen_window", False, None): ("flash_attention_extend_varlen_plan", "flash_attention_extend_varlen"),
    ("flash_attention_extend_varlen_window", True, None): ("flash_attention_extend_varlen_plan", "flash_attention_extend_varlen"),
    ("flash_attention_extend_varlen_window", False, WINDOW): ("flash_attention_extend_varlen_plan_window",
                                                              "flash_attention_extend_varlen_window"),
    ("flash_attention_extend_varlen_window", True, WINDOW): ("flash_attention_extend_varlen_plan_window",
                                                             "flash_attention_extend_varlen_window"),
    ("flash_attention_extend_paged_varlen", False, None): ("flash_attention_extend_varlen_plan", "flash_attention_extend_paged_varlen"),
    ("flash_attention_extend_paged_varlen", True, None): ("flash_attention_extend_varlen_plan", "flash_attention_extend_paged_varlen"),
    ("flash_attention_extend_paged_varlen_window", False, None): ("flash_attention_extend_varlen_plan",
                                                                  "flash_attention_extend_paged_varlen"),
    ("flash_attention_extend_paged_varlen_window", True, None): ("flash_attention_extend_varlen_plan",
                                                                 "flash_attention_extend_paged_varlen"),
    ("flash_attention_extend_paged_varlen_window", False, WINDOW): ("flash_attention_extend_varlen_plan_window",
                                                                    "flash_attention_extend_paged_varlen_window"),
    ("flash_attention_extend_paged_varlen_window", True, WINDOW): ("flash_attention_extend_varlen_plan_window",
                                                                   "flash_attention_extend_paged_varlen_window"),
}
# front -> the append entry point, whatever the cache type
APPEND = {
    "kv_cache_append": "flash_attention_kv_append",
    "kv_cache_append_paged": "flash_attention_kv_append_paged",
    "kv_cache_append_varlen": "flash_attention_kv_append_varlen",
    "kv_cache_append_paged_varlen": "flash_attention_kv_append_paged_varlen",
}


class Recorder:
    """``fa.lib()`` as the fronts see it: the real library, every attribute fetched from it noted by name"""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._real, name)


@pytest.fixture
def recorder(monkeypatch):
    rec = Recorder(fa.lib())
    monkeypatch.setattr(fa, "lib", lambda: rec)
    return rec


@functools.lru_cache(maxsize=None)
def tensors(fp8):
    """the caches of one cache type, contiguous and paged (a shuffled table), with their descales, and the lengths"""
    g = torch.Generator().manual_seed(4100 + fp8)
    K, V = (torch.randn(B, HKV, CAPACITY, D, generator=g).to(torch.bfloat16) for _ in range(2))
    ds = {}
    if fp8:
        K, V = K.to(torch.float8_e4m3fn), V.to(torch.float8_e4m3fn)
        ds = dict(k_descale=torch.tensor([0.75, 1.5]).to(DEV), v_descale=torch.tensor([1.25, 0.5]).to(DEV))
    n = CAPACITY // PAGE
    table = torch.randperm(B * n, generator=g).reshape(B, n).to(torch.int32)
    pools = []
    for T in (K, V):
        pool = torch.zeros(B * n, HKV, PAGE, D, dtype=torch.uint8 if fp8 else T.dtype)
        pool[table.reshape(-1).long()] = (T.view(torch.uint8) if fp8 else T).view(B, HKV, n, PAGE, D).transpose(1, 2).reshape(B * n, HKV, PAGE, D)
        pools.append((pool.view(torch.float8_e4m3fn) if fp8 else pool).to(DEV))
    return K.to(DEV), V.to(DEV), pools[0], pools[1], table.to(DEV), ds, torch.tensor(LENS, dtype=torch.int32).to(DEV)


@functools.lru_cache(maxsize=None)
def rows(seed, *shape):
    """bf16 rows of the given shape on the device: (B, heads, Sq, D), or token-packed (T, heads, D)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


CU = (0, ROWS[0], sum(ROWS))


@pytest.mark.parametrize("num_splits", [1, 2])
@pytest.mark.parametrize("front, fp8, window", sorted(ATTENTION, key=str), ids=lambda v: str(v).replace("flash_attention_", ""))
def test_attention_front_reaches_its_entry_point(recorder, front, fp8, window, num_splits):
    K, V, Kp, Vp, table, ds, lens = tensors(fp8)
    ragged, paged = "varlen" in front, "paged" in front
    if ragged:
        Q = rows(4200, sum(ROWS), H, D)
    else:
        Q = rows(4200, B, H, SQ_DECODE if "decode" in front else SQ_EXTEND, D)
    args = [Q, Kp, Vp, table] if paged else [Q, K, V]
    if ragged:
        args.append(torch.tensor(CU, dtype=torch.int32).to(DEV))
    kw = dict(ds, is_causal=True, num_splits=num_splits, return_lse=True)
    if "decode" in front or front.endswith("_window"):      # (the other fronts have no such argument)
        kw["window"] = window
    del recorder.names[:]
    O, lse = getattr(fa, front)(*args, lens, **kw)
    plan, launch = ATTENTION[front, fp8, window]
    assert recorder.names == [plan, WS, launch]
    torch.cuda.synchronize()
    assert O.shape == Q.shape and bool(torch.isfinite(O.float()).all()) and bool(torch.isfinite(lse).all())


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("front", sorted(APPEND))
def test_append_front_reaches_its_entry_point(recorder, front, fp8):
    K, V, Kp, Vp, table, ds, lens = (t.clone() if i < 4 else t for i, t in enumerate(tensors(fp8)))
    ragged, paged = "varlen" in front, "paged" in front
    shape = (sum(ROWS), HKV, D) if ragged else (B, HKV, SQ_EXTEND, D)
    Kn, Vn = rows(4300, *shape), rows(4301, *shape)
    args = [Kn, Vn, Kp, Vp, table] if paged else [Kn, Vn, K, V]
    if ragged:
        args.append(torch.tensor(CU, dtype=torch.int32).to(DEV))
    del recorder.names[:]
    assert getattr(fa, front)(*args, lens, **ds) is None
    assert recorder.names == [APPEND[front]]
    torch.cuda.synchronize()


def test_every_split_and_append_entry_point_is_reached():
    """the two tables name all fourteen split-KV entry points and all four append entry points the library exports"""
    split = {s for s in fa.EXPORTS if s.startswith(("flash_attention_decode", "flash_attention_extend"))
             and "plan" not in s and "workspace" not in s}
    assert len(split) == 14 and {launch for _, launch in ATTENTION.values()} == split
    assert set(APPEND.values()) == {s for s in fa.EXPORTS if s.startswith("flash_attention_kv_append")}
