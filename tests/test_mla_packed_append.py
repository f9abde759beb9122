"""GPU tests of the packed latent-cache append: WHOLE sentinel-filled caches byte for byte against the reference
writer of the 656-byte row -- every form, lengths around the 16-position wave, the 64-position block and the page, both scale formats."""
import pytest
import torch

import kv_cache_check as kc
import mla_check as mc
from kv_cache_check import DEV, fa

pytestmark = pytest.mark.gpu
CAP, B, ROW, FORMS = mc.CAPACITY, mc.B, 656, (0,) + mc.PAGES
parts = lambda t: (t[..., :mc.DL], t[..., mc.DL + 16:mc.DL + 16 + mc.DR])      # c_kv and k_pe: strided slices of one projection


def write(c, r, pow2=False):
    """bf16 c [.., 512], r [.., 64] -> uint8 [.., 656]: per block amax floored at 1e-4, scale amax * fl32(1 / 448) (pow2: rounded up to a
    power of two), the fp32 quotient clamped to +-448 and cast once to e4m3fn, the rope bytes copied"""
    x = c.float().reshape(*c.shape[:-1], 4, 128)
    s = x.abs().amax(-1).clamp_min(torch.tensor(1e-4)) * torch.tensor(1.0 / 448.0)
    if pow2:
        u = s.view(torch.int32)
        s = (((u >> 23) + ((u & 0x7FFFFF) != 0)) << 23).view(torch.float32)
    codes = (x / s[..., None]).clamp(-448, 448).to(kc.F8).view(torch.uint8).reshape(*c.shape[:-1], 512)
    return torch.cat([codes, s.contiguous().view(torch.uint8), r.contiguous().view(torch.uint8)], -1)


def projection(Sq, seed):
    """bf16 [B, Sq, 576 + 32].  Row 0: block 1 all zero (the amax floor), block 2 holding +amax and -amax (+-448 s before rounding:
    whether the quotient passes 448 is the scale's rounding) among small values and -0, block 3 with amax 448 and a bf16 subnormal"""
    proj = kc.randn((B, Sq, mc.D + 32), seed, torch.bfloat16)
    proj[:, 0, 128:256] = 0
    proj[:, 0, 256:384] = torch.tensor([3.171875, -3.171875, 3.15625, -0.0, 1e-3, 0.0, 1.0, -2.5], dtype=torch.bfloat16).repeat(16)
    proj[:, 0, 384:512] = torch.tensor([448.0, -7.0, 0.5, 1e-40], dtype=torch.bfloat16).repeat(32)
    return proj


def check(proj, lens, fmt, page, table=None):
    """append to a sentinel-filled cache or pool and compare every byte: the writer's rows at mla_append's positions, the rows of a table
    entry outside the pool dropped, the sentinel everywhere else"""
    Sq, new = proj.shape[1], write(*parts(proj), fmt == "pow2")
    cache = torch.full((B * (CAP // page) + 5, page, ROW) if page else (B, CAP, ROW), 0xA5, dtype=torch.uint8)
    want, dev, tab, pg = cache.clone(), cache.to(DEV), (table if page else torch.arange(B)[:, None]), page or CAP
    for b, L in enumerate(min(L, CAP) for L in lens):
        for p in range(max(L - Sq, 0), max(L, 0)):
            if 0 <= tab[b, p // pg] < len(cache):
                want[tab[b, p // pg], p % pg] = new[b, p - L + Sq]
    if page:
        fa.mla_cache_append_paged_packed(*parts(proj.to(DEV)), dev, table.to(DEV), kc.i32(lens), scale_fmt=fmt)
    else:
        fa.mla_cache_append_packed(*parts(proj.to(DEV)), dev, kc.i32(lens), scale_fmt=fmt)
    assert not torch.equal(want, cache) and torch.equal(dev.cpu(), want), (lens, (dev.cpu() != want).nonzero()[:4].tolist())


@pytest.mark.parametrize("Sq", [1, 5, 16, 70])           # 70: across a 64-position block and the 16-position waves, from an unaligned start
@pytest.mark.parametrize("page", FORMS)
@pytest.mark.parametrize("fmt", ["f32", "pow2"])
def test_every_byte_of_the_cache_after_the_append(fmt, page, Sq):
    proj, pg = projection(Sq, 7500 + Sq), page or 128
    for lens in ([0, max(Sq - 1, 1), CAP + 5], [pg - 1, pg, pg + 1], [-3, CAP, 2 * pg + 7], [15, 17, 65]):
        check(proj, lens, fmt, page, mc.table_for(B, page, 85 + Sq) if page else None)


def test_a_table_entry_outside_the_pool_skips_its_rows_and_nothing_else():
    wild = mc.table_for(B, 16, 86)                         # Sq 40 at length 100: positions 60 .. 99, pages 3 .. 6 of every sequence
    wild[0, 4], wild[1, 5] = -1, B * (CAP // 16) + 5
    check(projection(40, 7600), [100] * B, "f32", 16, wild)
