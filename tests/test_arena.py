"""CPU: the guarded arena of tests/arena.py refuses what it is meant to refuse.  The arena is run on CPU tensors: placements hold for
every dtype the suite uses, a clean arena passes, one byte planted directly before a view, directly behind it, far behind the last
view or inside an input is refused with the right tensor name and signed offset, and a write inside a writable view is not flagged."""
import pytest

torch = pytest.importorskip("torch")

import arena as ar  # noqa: E402

FP8 = getattr(torch, "float8_e4m3fn", None)
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.uint8] + ([FP8] if FP8 is not None else [])
RESIDUES = [ar.ALIGNED, ar.OFFSET, ar.SIDE, (8, 16), (0, 16), (240, 256)]


def small():
    """an arena with an input, an output, a strided input and a side input; returns (arena, views)"""
    arena, v = ar.Arena.of("cpu", {
        "Q": dict(shape=(2, 3, 5, 8), dtype=torch.bfloat16),
        "O": dict(shape=(2, 3, 5, 8), dtype=torch.float32, writable=True),
        "K": dict(shape=(1, 2, 7, 8), dtype=torch.bfloat16, strides=(7 * 2 * 8, 8, 2 * 8, 1)),      # the view of a (1, 7, 2 * 8) buffer
        "lens": dict(shape=(3,), dtype=torch.int32, residue=ar.SIDE),
    })
    g = torch.Generator().manual_seed(1)
    arena.load(v["Q"], torch.randn(2, 3, 5, 8, generator=g).bfloat16())
    arena.load(v["K"], torch.randn(1, 2, 7, 8, generator=g).bfloat16())
    arena.load(v["lens"], torch.tensor([1, 129, 300], dtype=torch.int32))
    return arena, v


@pytest.mark.parametrize("dtype,residue", [(t, r) for t in DTYPES for r in RESIDUES if r[0] % ar.itemsize(t) == 0], ids=str)
def test_residues_hold_for_every_dtype(dtype, residue):
    r, m = residue
    arena = ar.Arena("cpu", 3 * ar.footprint((3, 5, 16), dtype, residue))
    views = [arena.carve((3, 5, 16), dtype, residue, writable=i == 1, name=f"t{i}") for i in range(3)]
    for v in views:
        assert v.data_ptr() % m == r and v.dtype == dtype and v.shape == (3, 5, 16) and v.is_contiguous()
        assert bool((ar.bits(v) == (ar.FILL if v.element_size() == 1 else -1)).all()), "a fresh view is all 0xFF"
    lo = [v.data_ptr() - arena.base for v in views]
    hi = [a + v.numel() * v.element_size() for a, v in zip(lo, views)]
    assert lo[0] >= ar.BAND and all(b - a >= ar.BAND for a, b in zip(hi, lo[1:])) and arena.size - hi[-1] >= ar.TAIL
    arena.check()


def test_the_fill_reads_as_nan_and_minus_one():
    arena = ar.Arena("cpu", 4 * ar.footprint((8,), torch.float32))
    assert torch.isnan(arena.carve((8,), torch.float32)).all() and torch.isnan(arena.carve((8,), torch.bfloat16).float()).all()
    assert bool((arena.carve((8,), torch.int32, ar.SIDE) == -1).all())
    if FP8 is not None:
        assert torch.isnan(arena.carve((16,), FP8).float()).all()


def test_views_are_contiguous_or_carry_the_requested_strides():
    arena, v = small()
    assert v["Q"].is_contiguous() and v["O"].is_contiguous() and v["lens"].is_contiguous()
    assert v["K"].stride() == (112, 8, 16, 1) and not v["K"].is_contiguous()
    for name in ("Q", "O", "K"):
        assert v[name].data_ptr() % 256 == 16
    assert v["lens"].data_ptr() % 16 == 4
    model = v["K"].transpose(1, 2).reshape(1, 7, 16)          # the model-layout buffer behind the view
    assert model.data_ptr() == v["K"].data_ptr()
    assert v["lens"].tolist() == [1, 129, 300]


def test_a_clean_arena_passes_and_writable_views_may_change():
    arena, v = small()
    arena.check()
    v["O"].fill_(3.0)
    v["O"][1, 2, 4, 7] = float("nan")
    arena.check()
    arena.refill(v["O"])
    assert torch.isnan(v["O"]).all()
    arena.check()


def start(arena, view):
    return view.data_ptr() - arena.base


@pytest.mark.parametrize("name", ["Q", "O", "K", "lens"])
def test_one_byte_before_and_behind_a_view_is_refused(name):
    arena, v = small()
    a, n = start(arena, v[name]), ar.extent(v[name].shape, v[name].stride()) * v[name].element_size()
    for at, offset in ((a - 1, -1), (a + n, n)):
        arena.bytes[at] = 0
        with pytest.raises(ar.ArenaError) as e:
            arena.check()
        assert (e.value.name, e.value.offset, e.value.kind, e.value.count) == (name, offset, "outside", 1), str(e.value)
        assert ("before its start" if offset < 0 else "1 bytes past its end") in str(e.value)
        arena.bytes[at] = ar.FILL
        arena.check()


def test_a_byte_far_behind_the_last_view_is_refused():
    arena, v = small()
    a, n = start(arena, v["lens"]), 12
    far = a + n + 100 * 1024
    assert far < arena.size
    arena.bytes[far] = 0x7F
    with pytest.raises(ar.ArenaError) as e:
        arena.check()
    assert (e.value.name, e.value.offset, e.value.kind) == ("lens", n + 100 * 1024, "outside")
    arena.bytes[far] = ar.FILL
    arena.bytes[arena.size - 1] = 0                             # the very last byte of the tail
    with pytest.raises(ar.ArenaError) as e:
        arena.check()
    assert e.value.name == "lens" and e.value.offset == arena.size - 1 - a


def test_a_write_into_an_input_is_refused():
    arena, v = small()
    v["Q"][1, 0, 2, 3] += 1.0
    with pytest.raises(ar.ArenaError) as e:
        arena.check()
    at = ((1 * 3 + 0) * 5 + 2) * 8 + 3
    assert (e.value.name, e.value.kind) == ("Q", "input") and e.value.offset // 2 == at
    arena, v = small()
    v["lens"][2] = 301
    with pytest.raises(ar.ArenaError) as e:
        arena.check()
    assert (e.value.name, e.value.offset, e.value.kind) == ("lens", 8, "input")
    # an input that nothing was loaded into must stay 0xFF
    arena = ar.Arena("cpu", ar.footprint((4, 4), torch.float32))
    x = arena.carve((4, 4), torch.float32, name="X")
    x[3, 3] = 0.0
    with pytest.raises(ar.ArenaError) as e:
        arena.check()
    assert (e.value.name, e.value.offset, e.value.kind) == ("X", 60, "input")


def test_a_gap_between_the_rows_of_a_strided_view_is_checked():
    """a writable view of every second row: the rows between belong to no view"""
    arena = ar.Arena("cpu", ar.footprint((4, 8), torch.float32, strides=(16, 1)))
    x = arena.carve((4, 8), torch.float32, strides=(16, 1), writable=True, name="X")
    x.fill_(1.0)
    arena.check()
    wide = torch.as_strided(x, (4, 16), (16, 1))[:3]
    wide[1, 8] = 2.0                                            # the first element behind row 1
    with pytest.raises(ar.ArenaError) as e:
        arena.check()
    assert (e.value.name, e.value.offset, e.value.kind) == ("X", (16 + 8) * 4, "outside")


def test_the_arena_is_sized_by_its_carvings():
    arena, v = small()
    total = sum(ar.footprint(t.shape, t.dtype, ar.SIDE if n == "lens" else ar.OFFSET, t.stride()) for n, t in v.items())
    assert arena.size == ar.BAND + total + ar.TAIL
    with pytest.raises(AssertionError, match="arena too small"):
        arena.carve((1 << 20,), torch.uint8)
    with pytest.raises(AssertionError, match="cannot hold"):
        arena.carve((4,), torch.float32, (2, 16))
