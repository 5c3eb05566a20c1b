"""recip32 / recip32_exact_below (csrc/mgx_aux_geom.h): the one division-by-multiplication the streaming kernels, the pool restart, the
granule producers and the renderer use -- __umulhi(n, recip32(d)) for n / d -- against Python's integers, through the host shim (the
SAME functions the launchers call).  Every call site's divisor range has the bound it needs, the bound is tight where it says so, and
granule_geometry ends the batch where the quotient would go wrong."""
import numpy as np
import pytest

from multigrid_amd import _lib
from tests import hostshim

TWO32 = 1 << 32


def umulhi(n, m):
    return (n * m) >> 32


#: call site -> (its divisors, the dividends it forms stay below this)
SITES = {
    "one_hot: o / D": (range(3, 33), lambda d: 1 << 20),
    "full_obs: i / HW": (range(9, 65536), lambda d: 1 << 16),
    "full_obs: r / W, r / H": (range(3, 256), lambda d: 1 << 16),
    "copy_layouts: k / units": (range(2, 64), lambda d: 4096),
    "copy_layouts: k / A": (range(2, 33), lambda d: 2048),
    # mgx_render.hip, render_kernel: the dividend is a byte offset inside one pixel row of the band, o - py * R or bx, both < R =
    # W * 3 * ts with W <= 255 (mgx_render refuses wider grids): at most 255 * d - 1
    "render: offset / (3 * ts)": ([3 * ts for ts in range(1, 65)], lambda d: 255 * d),
}


@pytest.mark.parametrize("site", list(SITES))
def test_every_call_sites_range_is_exact(site):
    ds, below = SITES[site]
    for d in ds:
        m = hostshim.recip32(d)
        assert 0 <= m * d - TWO32 < d, f"{site}: recip32({d}) = {m} is not ceil(2^32 / {d})"
        assert hostshim.recip32_exact_below(d) >= below(d), f"{site}: d = {d}"


def test_granule_divisors():
    for gpe in range(2, 9):
        assert 0 <= hostshim.recip32(gpe) * gpe - TWO32 < gpe


def test_the_bound_is_what_the_header_derives():
    """e = recip32(d) * d - 2^32;  e == 0 ? 2^32 : ceil(2^32 / e) -- and below it the quotient IS right: every n for the small sites,
    the worst residue (n = d - 1 mod d) next to the bound for the others"""
    for d in list(range(2, 300)) + [1000, 4097, 65535, 65536, 65537, (1 << 31) - 1]:
        e = hostshim.recip32(d) * d - TWO32
        want = TWO32 if e == 0 else -(-TWO32 // e)
        assert hostshim.recip32_exact_below(d) == want, d
        m = hostshim.recip32(d)
        top = min(want, TWO32) - 1
        for n in {0, d - 1, d, top, top - top % d - 1, top - top % d}:
            if 0 <= n <= top:
                assert umulhi(n, m) == n // d, (d, n)
    for d in range(2, 64):                                   # every dividend the small sites can form
        n = np.arange(1 << 16, dtype=np.uint64)
        assert np.array_equal((n * np.uint64(hostshim.recip32(d))) >> np.uint64(32), n // np.uint64(d)), d


def test_the_bound_is_tight_where_it_is_below_2_32():
    for d, bound in ((5, 1 << 30), (7, 1431655766)):
        m = hostshim.recip32(d)
        assert hostshim.recip32_exact_below(d) == bound
        assert umulhi(bound - 1, m) == (bound - 1) // d
        wrong = bound + (d - 1 - bound % d) % d              # the first n = d - 1 (mod d) at or above the bound
        assert umulhi(wrong, m) == wrong // d + 1, (d, wrong)
    assert umulhi(1 << 30, hostshim.recip32(5)) == 214748365 and (1 << 30) // 5 == 214748364
    assert umulhi(1431655770, hostshim.recip32(7)) != 1431655770 // 7
    for d in (2, 3, 4, 6, 8):
        assert hostshim.recip32_exact_below(d) >= 1 << 31


def test_granule_geometry_ends_the_batch_where_the_quotient_would_go_wrong():
    """The limit on the granules in all: 2^31 for 1, 2, 3, 4, 6, 8 granules per env, 2^30 for 5 (17..20 agents), 1 431 655 766 for 7
    (25..28 agents).  (The granules in all are a multiple of the granules per env, so the limit itself need not be one: the first
    batch that reaches it is refused, the one before is accepted.)"""
    limits = {1: 1 << 31, 2: 1 << 31, 3: 1 << 31, 4: 1 << 31, 6: 1 << 31, 8: 1 << 31, 5: 1 << 30, 7: 1431655766}
    for A in range(1, 33):
        gpe = (A + 3) // 4
        first = -(-limits[gpe] // gpe)                       # the first batch whose granules reach the limit
        rc, g, inv, ng = hostshim.granule_geometry(A, first)
        assert rc == _lib.ERR_UNSUPPORTED and g == gpe and ng == first * gpe >= limits[gpe], A
        rc, g, inv, ng = hostshim.granule_geometry(A, first - 1)
        assert rc == 0 and ng == (first - 1) * gpe < limits[gpe], A
        assert inv == (hostshim.recip32(gpe) if gpe > 1 else 0)
        if gpe > 1:                                          # ... and every granule index an accepted batch has divides exactly
            for n in (ng - 1, ng - gpe, ng - ng % gpe - 1):
                assert umulhi(n, inv) == n // gpe, (A, n)
    assert hostshim.granule_geometry(20, 214748365)[0] == _lib.ERR_UNSUPPORTED        # 2^30 + 1 granules
    assert hostshim.granule_geometry(20, 214748364)[0] == 0
    assert hostshim.granule_geometry(28, 204522253)[0] == _lib.ERR_UNSUPPORTED        # 1 431 655 771 granules
    assert hostshim.granule_geometry(28, 204522252)[0] == 0
    assert hostshim.granule_geometry(0, 4)[0] == _lib.ERR_INVALID_ARGUMENT and hostshim.granule_geometry(33, 4)[0] == _lib.ERR_INVALID_ARGUMENT
    assert hostshim.granule_geometry(4, 0)[0] == _lib.ERR_INVALID_ARGUMENT
