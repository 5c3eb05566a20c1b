"""A census of the paths of the persistent hand-shake's producer kernels (csrc/mgx_aux.hip: persistent_post_kernel,
persistent_wait_kernel, persistent_feed_kernel<4|2|1|0>) that the GPU cases of tests/persist_cases.py reach -- on the CPU.

Which path a shape takes is decided by launch arithmetic alone: the feed's workgroup count and slice length (csrc/mgx_aux_geom.h:
feed_geometry), the granule arithmetic (granule_geometry) and the wait's pass of 8 x 256 flags.  This test takes that arithmetic from
the launchers' own header through tests/hostshim -- not from a Python copy of it --, walks every workgroup of every case and asserts
that (a) each case still has the launch and reaches the paths it was written for and (b) every path listed here is reached by some
case.  When the launch policy changes, this fails and points at the table: the fix is to tests/persist_cases.py, not to the
assertions (the same idea as tests/test_aux_branch_census.py).

One path of the feed kernel no launch reaches, and the test says so by walking the header's arithmetic: a workgroup whose slice is
empty (`g_lo >= ng_all`).

The NumPy model's round trip through the consumer's extraction is here too."""
import numpy as np
import pytest

from tests import hostshim
from tests import persist_cases as pc


# ===================================================================================================================== feed
def feed_reached(case):
    """(the launch geometry, the labels the case reaches): persistent_feed_kernel's workgroup-uniform branches, per workgroup"""
    rc, gpe, _, ng_all = hostshim.granule_geometry(case.A, case.B)
    assert rc == 0 and gpe == pc.gpe_of(case.A)
    geo = hostshim.feed_geometry(ng_all)
    nwg, per_wg, chunk = geo["nwg"], geo["per_wg"], geo["slice"]
    gb = pc.feed_gb(case.A)
    reached = {f"GB {gb}"}
    if nwg == 1:
        reached.add("one workgroup")
    elif nwg == geo["max_wgs"]:
        reached.add("the cap of 32")
    else:
        reached.add("several workgroups")
    if -(-ng_all // nwg) % 2:
        reached.add("per_wg rounded up")
    beyond = False
    for i in range(nwg):
        g_lo = i * per_wg
        ng = min(per_wg, ng_all - g_lo)
        assert ng >= 1, "a workgroup without granules"
        if ng < per_wg:
            assert i == nwg - 1
            reached.add("short last workgroup")
        if gb:                                  # the register chunk, then `for (; gdone < ng; gdone += chunk)`
            rest = ng - min(ng, chunk)
            beyond |= rest > 0
            if rest >= chunk:
                reached.add("second chunk full")
            elif rest > 0:
                reached.add("second chunk partial")
            if rest > chunk:
                reached.add("third chunk")
        else:                                   # `for (g = threadIdx.x + gdone; g < ng; ...)` with gdone = 0
            reached.add("by-index tail at g_lo == 0" if g_lo == 0 else "by-index tail at g_lo > 0")
    if gb and not beyond:
        reached.add("register chunk only")
    return geo, reached


def test_feed_cases_reach_every_branch():
    union = set()
    for case, name in zip(pc.FEED, pc.FEED_IDS):
        geo, reached = feed_reached(case)
        print(f"feed {name}: {geo['nwg']} workgroups of {geo['per_wg']} granules reach {sorted(reached)}")
        assert (geo["nwg"], geo["per_wg"]) == (case.nwg, case.per_wg), \
            f"{name}: the launcher now takes {geo['nwg']} workgroups of {geo['per_wg']}: re-derive the case in tests/persist_cases.py"
        assert set(case.labels) <= reached, f"{name}: no longer reaches {sorted(set(case.labels) - reached)}"
        assert case.act_off % max(pc.feed_gb(case.A), 1) == 0, f"{name}: the launcher refuses this action offset"
        union |= set(case.labels)
    for label in pc.FEED_LABELS:
        assert label in union, f"no feed case is written for '{label}'"
    # what the cases were chosen for beyond the labels: the slices of (., 2049) and (., 67621), each width of load at both
    by = {(c.A, c.B): c for c in pc.FEED}
    for A in (4, 2, 1):
        assert 2049 - by[A, 2049].per_wg == 1023 and by[A, 67621].per_wg - 2048 == 66 and 67621 - 31 * by[A, 67621].per_wg == 2087
    assert {c.waves for c in pc.FEED} == {7, 2049} and {c.trace for c in pc.FEED} == {True, False}
    assert any(c.act_off for c in pc.FEED if pc.feed_gb(c.A) == 4) and any(c.act_off % 4 == 2 for c in pc.FEED if c.A == 2)
    assert any(c.act_off % 2 for c in pc.FEED if pc.feed_gb(c.A) == 1) and any(c.act_off % 2 for c in pc.FEED if pc.feed_gb(c.A) == 0)
    o = pc.OUTLIVE
    assert (o["A"], o["B"]) in by and o["done"] + 1 < o["T"]


def test_feed_constants_and_the_unreachable_empty_slice():
    """kFeedSlice etc. as the cases assume them; and no launch holds a workgroup with `g_lo >= ng_all`: every ng up to 200 000
    (which covers every launch below the cap of 32 workgroups, reached at 63 489, and the cap's first 136 000 sizes), and at the cap
    samples up to the granule limit.  (At the cap the last slice starts at 31 * per_wg <= 31 * (ng / 32 + 2), which is >= ng only
    for ng <= 1984.)"""
    geo = hostshim.feed_geometry(1)
    assert (geo["slice"], geo["threads"], geo["pre"], geo["max_wgs"]) == (2048, 256, 8, 32)
    assert hostshim.feed_first_empty_slice(1, 200_000) is None
    for top in (2 ** 20, 2 ** 24, 2 ** 31 - 1):                     # at the cap: 31 * per_wg < ng wherever it is looked at
        assert hostshim.feed_first_empty_slice(top - 4096, top) is None
    r = pc._rng("empty slice")
    for ng in r.integers(65_537, 2 ** 31, size=2000):
        g = hostshim.feed_geometry(int(ng))
        assert g["nwg"] == 32 and 31 * g["per_wg"] < ng <= 32 * g["per_wg"]
    # ... and the formulas themselves, restated once
    for ng in (1, 2047, 2048, 2049, 4097, 65_535, 65_536, 65_537, 140_001):
        g = hostshim.feed_geometry(ng)
        nwg = min(-(-ng // 2048), 32)
        assert (g["nwg"], g["per_wg"]) == (nwg, (-(-ng // nwg) + 1) & ~1)


# ===================================================================================================================== post
def post_reached(case):
    """persistent_post_kernel: one thread per granule, 256 per workgroup"""
    rc, gpe, inv, ng = hostshim.granule_geometry(case.A, case.B)
    assert rc == 0
    if gpe > 1:                                 # the quotient the kernel takes, on the last granule
        assert ((ng - 1) * inv) >> 32 == (ng - 1) // gpe and inv == hostshim.recip32(gpe)
    return {"gpe == 1" if gpe == 1 else "gpe > 1", "dword read" if case.A % 4 == 0 else "byte gather",
            "last block full" if ng % 256 == 0 else "last block ragged"}


def test_post_cases_reach_every_branch():
    union = set()
    for case, name in zip(pc.POST, pc.POST_IDS):
        reached = post_reached(case)
        assert set(case.labels) == reached, f"{name}: reaches {sorted(reached)}"
        assert case.act_off in pc.post_action_offsets(case.A) and case.gr_off in pc.POST_GRANULE_OFFSETS and case.tag in pc.POST_TAGS
        union |= reached
    assert union == set(pc.POST_LABELS)
    assert {c.A for c in pc.POST} == {1, 2, 3, 4, 5, 7, 8, 12, 16, 17, 25, 32}
    assert {pc.gpe_of(c.A) for c in pc.POST} == {1, 2, 3, 4, 5, 7, 8}             # (5 and 7: the reciprocals with a remainder)
    assert {c.B for c in pc.POST} == {1, 255, 256, 257, 1003}
    for A in {c.A for c in pc.POST}:
        mine = [c for c in pc.POST if c.A == A]
        assert len({c.B for c in mine}) >= 2, f"A = {A} at one batch only"
        assert {c.act_off for c in mine} == set(pc.post_action_offsets(A))
    # every tag and both granule offsets with the dword read and with the byte gather; the top bit of the tag at gpe > 1 as well
    for dword in (True, False):
        mine = [c for c in pc.POST if (c.A % 4 == 0) == dword]
        assert {c.tag for c in mine} == set(pc.POST_TAGS) and {c.gr_off for c in mine} == set(pc.POST_GRANULE_OFFSETS)
    assert any(c.tag == 2 ** 32 - 1 and pc.gpe_of(c.A) > 1 for c in pc.POST)
    assert len(set(pc.POST_IDS)) == len(pc.POST)


# ===================================================================================================================== wait
def wait_reached(waves):
    loads, threads, per_pass = hostshim.wait_geometry()
    assert (loads, threads, per_pass) == (8, 256, 2048)
    reached = set()
    if waves < 64:
        reached.add("under one wavefront")
    if waves % threads:
        reached.add("ragged 256 boundary")
    if waves == per_pass:
        reached.add("exactly one pass")
    if waves > per_pass:
        reached.add("second pass")
        if (waves - per_pass) % threads:
            reached.add("ragged second pass")
    return reached


def test_wait_cases_reach_every_branch():
    promised = {1: {"under one wavefront", "ragged 256 boundary"}, 63: {"under one wavefront", "ragged 256 boundary"},
                64: {"ragged 256 boundary"}, 255: {"ragged 256 boundary"}, 256: set(), 257: {"ragged 256 boundary"},
                2047: {"ragged 256 boundary"}, 2048: {"exactly one pass"}, 2049: {"second pass", "ragged second pass", "ragged 256 boundary"},
                4097: {"second pass", "ragged second pass", "ragged 256 boundary"}}
    assert tuple(promised) == pc.WAIT_WAVES
    union = set()
    for waves in pc.WAIT_WAVES:
        reached = wait_reached(waves)
        assert reached == promised[waves], f"waves {waves}: reaches {sorted(reached)}"
        union |= reached
        late = pc.wait_late_positions(waves)
        assert late[0] == 0 and late[-1] == waves - 1 and all(0 <= p < waves for p in late)
    assert union == set(pc.WAIT_LABELS)
    # the late flag sits on both sides of a 256-thread boundary and of the pass boundary somewhere
    assert {255, 256} <= set(pc.wait_late_positions(257)) and {2047, 2048} <= set(pc.wait_late_positions(2049))
    assert 4096 in pc.wait_late_positions(4097)                        # (a third pass: its only flag)


# ===================================================================================================================== the model
@pytest.mark.parametrize("A", range(1, 33))
def test_model_round_trip_through_the_consumers_extraction(A):
    r = pc._rng("round trip", A)
    a = pc.random_actions(r, (257, A))
    for tag in pc.POST_TAGS:
        g = pc.granules_reference(a, tag)
        assert g.shape == (257, pc.gpe_of(A)) and g.dtype == np.uint64
        got, tags = pc.decode(g, A)
        np.testing.assert_array_equal(got, a)
        assert (tags == tag).all()
        # ... whatever the ignored bytes hold
        noisy = g | ~pc.granule_mask(A)
        np.testing.assert_array_equal(pc.decode(noisy, A)[0], a)
        assert ((noisy & pc.granule_mask(A)) == g).all()
    # the words of include/mgx.h on one granule, by hand: agents 4..6 of a 7-agent env, tag 3
    if A == 7:
        one = np.array([[1, 2, 3, 4, -1, 5, -128]], np.int8)
        assert pc.granules_reference(one, 3).tolist() == [[(3 << 32) | 0x04030201, (3 << 32) | 0x008005FF]]
        assert pc.granule_mask(7).tolist() == [0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF00FFFFFF]
    assert 0.15 < (a == -1).mean() < 0.4 and a.min() < -100 and a.max() > 100
