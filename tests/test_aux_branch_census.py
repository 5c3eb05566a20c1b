"""A census of the paths of the streaming kernels (csrc/mgx_aux.hip) that the GPU cases of tests/aux_cases.py reach -- on the CPU.

one_hot, full_obs, pack / unpack / check_grid and reset_done choose between fast and slow paths by pointer alignment, by a group size
the launcher derives from the batch (full_obs: G envs per wavefront, halved until 4096 wavefronts exist) and by tail length.  Which
path a shape takes is decided by launch arithmetic alone, so it can be derived without a GPU: this test takes that arithmetic from the
launchers' own header (csrc/mgx_aux_geom.h, exported by tests/hostshim -- not from a Python copy of it), walks every wavefront of every
case and asserts that (a) each case still has the geometry and reaches the branches it was written for and (b) every branch listed
here is reached by some case.  When the launch policy changes, this fails and points at the table: the fix is to tests/aux_cases.py,
not to the assertions (the same idea as tests/test_step_path_census.py).

It also holds the inputs of the full_obs cases to their two conditions: the NumPy reference agrees with the oracle's per-env
FullyObsWrapper on 64 envs per case, and neighbouring envs do not share a grid (a cross-env indexing error would hide)."""
import numpy as np
import pytest

from tests import aux_cases as ac
from tests import hostshim

FULL_OBS_LABELS = ("G>1", "G max", "group crosses env", "output-ordered", "input-ordered", "<=3 leftover cells", "ragged last wave",
                   "pow2", "non-pow2", "cell_bytes 1", "cell_bytes 2", "cell_bytes 3", "eight-in-flight loop", "single loop",
                   "input-ordered four-in-flight loop", "input-ordered single loop")
G_MAX = 227                                     # 6144 / (3 * 3 * 3): the smallest grid the spec admits


def is_pow2(v):
    return v & (v - 1) == 0


def full_obs_reached(case):
    """(the launch geometry, the labels the case reaches): full_obs_kernel's wave-uniform branches, per wavefront"""
    W, H, cb, B = case.W, case.H, case.cb, case.B
    geo = hostshim.full_obs_geom(W, H, cb, B)
    G, HW = geo["G"], W * H
    w = np.arange(geo["nwaves"], dtype=np.int64)
    e0 = w * G
    Gc = np.minimum(G, B - e0)
    assert (Gc >= 1).all()
    oskew = (w * G * W * H * 3) % 16
    out_ord = oskew % 4 == 0                    # the wavefront's slice of the output starts on a dword: four output cells per lane
    ncell = Gc * HW
    ngrp = ncell // 4
    reached = set()
    if G > 1:
        reached |= {"G>1", f"cell_bytes {cb}"}
        reached |= {"output-ordered"} if out_ord.any() else set()
        reached |= {"input-ordered"} if (~out_ord).any() else set()
    if G == G_MAX:
        reached.add("G max")
    # a 4-cell group spans two envs: the `xx == W` wrap of gather4
    if (out_ord & (Gc > 1)).any() and HW % 4 != 0:
        reached.add("group crosses env")
    if (out_ord & (ncell % 4 != 0)).any():
        reached.add("<=3 leftover cells")
    if Gc[-1] < G:
        reached.add("ragged last wave")
    # the (env, x, y) decomposition: shifts when the sides allow (gather4: H and HW; move: W and HW), reciprocal multiplies otherwise
    if (out_ord.any() and is_pow2(H) and is_pow2(HW)) or ((~out_ord).any() and is_pow2(W) and is_pow2(HW)):
        reached.add("pow2")
    if (out_ord.any() and not (is_pow2(H) and is_pow2(HW))) or ((~out_ord).any() and not (is_pow2(W) and is_pow2(HW))):
        reached.add("non-pow2")
    # lane 0 of `for (k = lane; k + 64 < ngrp; k += 128)`, and whoever is left for `for (; k < ngrp; k += 64)`
    if (out_ord & (ngrp > 64)).any():
        reached.add("eight-in-flight loop")
    if (out_ord & (ngrp % 128 != 0)).any():
        reached.add("single loop")
    if (~out_ord & (ncell > 192)).any():
        reached.add("input-ordered four-in-flight loop")
    if (~out_ord & (ncell % 256 != 0)).any():
        reached.add("input-ordered single loop")
    return geo, reached


def test_full_obs_cases_reach_every_branch():
    union = set()
    for case, name in zip(ac.FULL_OBS, ac.FULL_OBS_IDS):
        geo, reached = full_obs_reached(case)
        print(f"full_obs {name}: {geo} reaches {sorted(reached)}")
        assert geo["G"] == case.G, f"{name}: the launcher now takes G = {geo['G']}: re-derive the case in tests/aux_cases.py"
        assert set(case.labels) <= reached, f"{name}: no longer reaches {sorted(set(case.labels) - reached)}"
        assert geo["wpb"] * geo["wave_lds"] <= 64 * 1024 and geo["in_buf"] >= case.G * case.W * case.H * case.cb + 31
        union |= set(case.labels)
    for label in FULL_OBS_LABELS:
        assert label in union, f"no full_obs case is written for '{label}'"
    print("full_obs: every label reached:", ", ".join(FULL_OBS_LABELS))
    # each cell format at G > 1, and each pass at G > 1
    for label in ("cell_bytes 1", "cell_bytes 2", "cell_bytes 3", "output-ordered", "input-ordered"):
        assert any(label in c.labels and c.G > 1 for c in ac.FULL_OBS)
    # what no shape reaches: the input-ordered pass with the shift decomposition -- W * H a power of two >= 16 makes every wavefront's
    # output offset a multiple of 48 bytes, i.e. of 16
    for W in range(3, 256):
        for H in range(3, 256):
            if is_pow2(W) and is_pow2(W * H):
                assert (W * H * 3) % 16 == 0


def test_full_obs_bench_form_is_a_case():
    """bench.py --full times 16x16, 16-bit cells at G = 8; that form's bytes are checked at a cell count that is no multiple of four"""
    case = next(c for c in ac.FULL_OBS if (c.W, c.H, c.cb) == (16, 16, 2))
    assert hostshim.full_obs_geom(16, 16, 2, 1 << 20)["G"] == case.G == 8
    assert (case.B * 256) % (case.G * 256) != 0 and case.B % 4 != 0


@pytest.mark.parametrize("case", ac.FULL_OBS, ids=ac.FULL_OBS_IDS)
def test_full_obs_inputs_and_reference(case):
    from multigrid_amd import layouts
    from oracle import binding as ob
    cells, g3, ag = ac.full_obs_inputs(case)
    same = (cells[1:] == cells[:-1]).reshape(case.B - 1, -1).all(1)
    assert same.mean() <= 0.01, f"{same.sum()} consecutive env pairs share a grid"
    # agents: stacked, and some out of range
    pos = ag[..., 2].astype(int) * 256 + ag[..., 3]
    if case.A > 1:
        assert (pos[:, 1:] == pos[:, :1]).any(1).mean() > 0.3
    outside = (ag[..., 2] >= case.W) | (ag[..., 3] >= case.H)
    assert 0.01 < outside.mean() < 0.06
    if case.cb != 1:
        assert ((g3[..., 0] == ac.T_BOX) & (g3[..., 2] > 3)).mean() > 0.02            # filled boxes, whose content must be masked
    # the reference against the oracle's FullyObsWrapper, env by env: the first and the last envs, agents moved into range
    sel = np.r_[0:ac.ORACLE_ENVS // 2, case.B - ac.ORACLE_ENVS // 2:case.B]
    a_in = ag[sel].copy()
    a_in[..., 2] %= case.W
    a_in[..., 3] %= case.H
    shown = g3[sel].copy()
    shown[..., 2] &= 3
    got = ac.full_obs_reference(g3[sel], a_in)
    for k in range(len(sel)):
        want = ob.full_obs(layouts.grid_from_product(shown[k]), layouts.unpack_agents(a_in[k]))
        np.testing.assert_array_equal(got[k], want.astype(np.uint8))
    # ... and out-of-range rows write nothing: the same image as without them
    full = ac.full_obs_reference(g3[sel], ag[sel])
    for k in range(len(sel)):
        inside = ~outside[sel[k]]
        want = ob.full_obs(layouts.grid_from_product(shown[k]), layouts.unpack_agents(ag[sel[k]][inside])) if inside.any() \
            else layouts.grid_from_product(shown[k])
        np.testing.assert_array_equal(full[k], want.astype(np.uint8))


def test_one_hot_cases_reach_every_branch():
    cells_per_chunk, chunks, blocks = hostshim.one_hot_geom(ac.ONE_HOT_BIG[0])
    assert cells_per_chunk == 1024
    assert chunks > blocks == 4096, "the big case no longer runs the grid-stride loop"
    assert ac.ONE_HOT_BIG[0] % 1024 not in (0,) and ac.ONE_HOT_BIG[0] % 4 != 0           # a ragged last chunk, a ragged last thread
    assert ac.ONE_HOT_BIG[0] * (3 + sum(ac.ONE_HOT_BIG[1])) < 13 * 2 ** 20 * 2
    ns = set(ac.ONE_HOT_N)
    assert {1023, 1024, 1025} <= ns and {2047, 2048, 2049} <= ns                       # around one chunk, around two
    assert any(hostshim.one_hot_geom(n)[1] == 1 for n in ns) and any(hostshim.one_hot_geom(n)[1] == 3 for n in ns)
    dims = ac.one_hot_dims()
    assert len(set(dims)) == len(dims) and (11, 6, 4) in dims
    assert {sum(d) for d in dims} == set(ac.ONE_HOT_D) and max(ac.ONE_HOT_D) == 32      # bit 31 of the mask
    for D in ac.ONE_HOT_D:
        assert sum(1 for d in dims if sum(d) == D) == (D - 1) * (D - 2) // 2            # every composition into three parts
    for d in ac.ONE_HOT_SWEEP_DIMS:
        assert d in dims


def test_pack_cases_reach_every_branch():
    """one thread converts 8 cells: whole and ragged octets, one and several workgroups, octets that span rows and envs"""
    assert {7, 8, 9} <= set(ac.PACK_N) and {2047, 2048, 2049} <= set(ac.PACK_N)
    spans_env = spans_row = ragged = blocks = False
    for W, H, B in ac.PACK_ENV:
        n = W * H * B
        spans_env |= W * H < 16 and B > 1 and (W * H) % 8 != 0
        spans_row |= W < 8
        ragged |= n % 8 != 0
        blocks |= n > 2048
    assert spans_env and spans_row and ragged and blocks
    assert {(3, 3), (3, 4), (5, 3)} <= {(W, H) for W, H, B in ac.PACK_ENV}


def test_check_cases_reach_every_branch():
    rows_outnumber = octets_outnumber = False
    for c in ac.CHECK:
        octets, rows = (c.W * c.H * c.B + 7) // 8, c.A * c.B
        rows_outnumber |= rows > octets
        octets_outnumber |= octets > rows
        cells, ag = ac.check_inputs(c)
        for name, m in ac.cell_defects(cells, c.cb).items():
            assert m.sum() >= 8, f"{c}: cell defect '{name}' planted {m.sum()} times"
        for name, m in ac.agent_defects(ag, c.W, c.H, c.cb).items():
            assert m.sum() >= 4, f"{c}: agent defect '{name}' planted {m.sum()} times"
        ring = ac.ring_mask(c.H, c.W)[None] & (cells != (0xD2 if c.cb == 1 else 0x8502))
        assert ring.sum() >= 8
        assert set(ac.cell_defects(cells, c.cb)) == set(ac.CELL_CLASSES8 if c.cb == 1 else ac.CELL_CLASSES16)
        assert set(ac.agent_defects(ag, c.W, c.H, c.cb)) == set(ac.AGENT_CLASSES)
        clean = ac.valid_state(ac._rng("clean", *c), c.W, c.H, c.A, c.B, c.cb)
        assert ac.check_reference(*clean, c.W, c.H, c.cb) == [0, 0, 0, 2 ** 31 - 1]
    assert rows_outnumber and octets_outnumber
    assert any((c.W, c.H, c.A) == (3, 3, 32) for c in ac.CHECK)


def test_reset_cases_reach_every_copy_unit():
    """the copy units {16, 8, 4, 2, 1} against `units < 64` (flattened over the lanes) and `units >= 64` (env by env)"""
    reached = set()
    for c, name in zip(ac.RESET, ac.RESET_IDS):
        env_bytes = c.W * c.H * c.cb
        unit, units = hostshim.reset_unit(env_bytes, 0, c.pool_off)            # (the tensors themselves sit on 256-byte boundaries)
        assert (unit, units >= 64) == (c.unit, c.big), f"{name}: the launcher now copies {units} units of {unit} bytes"
        assert unit * units == env_bytes
        if c.pool_off:
            assert hostshim.reset_unit(env_bytes, 0, 0)[0] > unit, f"{name}: the offset no longer degrades the unit"
        reached.add((unit, units >= 64))
    missing = {(u, big) for u in (16, 8, 4, 2, 1) for big in (False, True)} - reached
    assert not missing, f"no reset_done case copies in (unit, units >= 64) = {sorted(missing)}"
    assert {c.A for c in ac.RESET} >= {1, 3, 4} and {c.K for c in ac.RESET} == {1, 7}
    assert any(c.first_env == 2 ** 40 + 5 for c in ac.RESET) and any(c.aux for c in ac.RESET) and any(c.pool_off for c in ac.RESET)
    assert any(c.cb == 1 and c.A == 1 for c in ac.RESET)                        # (one agent: the `units == 1` division)
    for c in ac.RESET:
        st = ac.reset_inputs(c)
        done = ac.reset_reference(st, c)[1]
        assert 0.3 < done.mean() < 0.5 and c.B % 64 != 0 and c.B > 256


def test_valid_masks_are_what_the_host_packers_accept():
    """valid16 / valid8 (include/mgx.h's words, what bad[0] is counted from) against layouts.pack_cells / pack_cells8, cell by cell; and
    the compact cases hold cells that break several rules at once -- bad[0] counts cells, not rules"""
    from multigrid_amd import layouts
    r = ac._rng("valid masks")
    g = ac.pack_cells3(r, (3000,))
    g[:4] = [(4, 1, 3), (4, 1, 2), (10, 2, 3), (12, 0, 0)]                  # a door's state 3 would read back as an agent overlay
    for mask, pack in ((ac.valid16(g), layouts.pack_cells), (ac.valid8(g), layouts.pack_cells8)):
        assert 0.15 < mask.mean() < 0.7                                      # (both outcomes well represented)
        for cell, ok in zip(g, mask):
            try:
                pack(cell[None])
                accepted = True
            except ValueError:
                accepted = False
            assert accepted == bool(ok), (cell.tolist(), pack.__name__)
    assert ac.valid8(g[:4]).tolist() == [False, True, True, False] and ac.valid16(g[:4]).all()
    t, sb = g[:, 0].astype(int), g[:, 2].astype(int)
    rules = ((~ac.valid16(g)).astype(int) + ((sb >> 2) != 0) + (((sb & 3) != 0) & (t != ac.T_DOOR) & (t != ac.T_AGENT)) + ((t > 10) & (t < 16)))
    assert (rules >= 2).sum() > 100
