"""Walking-distance fields on the GPU: distance_kernel (csrc/mgx_distance.hip) against the NumPy statement of the rule in
tests/test_distance.py, bit for bit, for `field` and `agent_dist` -- first through the backend on synthetic state sets of random
grids (walls at density 0.3, doors of all three states, objects, lava, goals; every member a view one row into a larger allocation,
the outputs between guard words), in the three cell formats, at the smallest shapes that reach every lane-group size of the launch
geometry (csrc/mgx_aux_geom.h: distance_geom; `geometry` restates it and tests/test_distance.py holds the restatement to the header),
with one env, one env short of two wavefronts and one env over; then the named cases; then through BatchedMultiGridEnv and EnvSnapshot
on small real envs, against the model of an oracle-backed twin.

The random cases are made by `random_case` from the seeds written below; `test_the_random_cases_are_not_hollow` (no GPU) asserts on
the model alone that they hold unreachable passable cells, envs without a source, floods deeper than H + W and sources on impassable
cells."""
import ctypes as C

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib, layouts
from multigrid_amd.constants import Type
from tests import util
from tests.test_distance import (AVOID_LAVA, DOOR, EMPTY, GOAL, KEY, LAVA, THROUGH_CLOSED, THROUGH_LOCKED, THROUGH_OBJECTS, WALL, DistOracle,
                                 agents_at, geometry, model_distance, model_passable, model_sources, random_grids, random_query, spec_for)
from tests.test_env_snapshot import make_env
from tests.test_episode_stats import actions_for
from tests.test_state_key import cell_bytes_of

gpu = pytest.mark.gpu
DEV = "cuda:0"
INT32_MAX = 2 ** 31 - 1
FILL = 0x7777

#: (H, W): what each reaches is in the names
FORMAT = {1: "compact", 2: "16bit", 3: "bytes"}
SHAPES = {"3x3_group4": (3, 3), "5x4_idle_lanes": (5, 4), "7x6_idle_lanes": (7, 6), "8x8": (8, 8), "16x16": (16, 16), "17x9_group32": (17, 9),
          "33x64_group64": (33, 64), "64x3": (64, 3), "64x64": (64, 64)}
CASES = [(shape, cb, A) for k, shape in enumerate(SHAPES) for cb in (2, 1, 3) for A in ((1, 4)[(k + cb) % 2],)] + [("8x8", cb, 32) for cb in (2, 1, 3)]
#: the seed of each random case: its position in CASES plus this
SEED0 = 100


def backend(spec):
    from multigrid_amd.ops import HipBackend
    return HipBackend(spec, torch.device(DEV))


def pack(cb, g):
    return np.ascontiguousarray(g if cb == 3 else (layouts.pack_cells8(g) if cb == 1 else layouts.pack_cells(g)))


def random_case(case):
    """(spec, rows, the states {"cells", "agents"}, three queries) of one random case: two wavefronts' envs and one more.  The first
    query is whatever random_query draws; the second has ONE point per env and nothing else (a flood from one cell runs deep); the
    third is types alone.  Envs 1 mod 5 of the point queries have their points outside the grid: no source."""
    shape, cb, A = case
    H, W = SHAPES[shape]
    r = np.random.default_rng(SEED0 + CASES.index(case))
    rows = 2 * geometry(W, H, 1)[1] + 1
    st = random_grids(r, rows, W, H, A, cb)
    q0 = random_query(r, rows, W, H, A)
    q0["points"][1::5] = (-1, H)
    one = np.stack((r.integers(0, W, size=(rows, 1)), r.integers(0, H, size=(rows, 1))), axis=-1).astype(np.int16)
    one[1::5] = (W, 0)
    q1 = dict(points=np.ascontiguousarray(one), flags=int(r.integers(0, 16)))
    q2 = dict(type_mask=1 << GOAL | 1 << KEY, colour_mask=int(r.integers(1, 64)), flags=int(r.integers(0, 16)))
    return spec_for(W, H, A, cb), rows, st, (q0, q1, q2)


def census_of(cb, st, spec, q):
    """what the model says of a query over a state set: envs with unreachable passable cells / without a source / deeper than H + W /
    with a source on an impassable cell"""
    d, _ = model_distance(cb, st["cells"], st["agents"], spec, **q)
    src, t, s = model_sources(cb, st["cells"], st["agents"], spec, q.get("type_mask", 0), q.get("colour_mask", 0xFF), q.get("agent_mask", 0),
                              q.get("points"))
    passable = model_passable(t, s, q.get("flags", 0))
    has = src.any(axis=(1, 2))
    return np.array([int((has & (passable & (d < 0)).any(axis=(1, 2))).sum()), int((~has).sum()),
                     int((d.max(axis=(1, 2)) > spec.width + spec.height).sum()), int((src & ~passable).any(axis=(1, 2)).sum())])


def test_the_random_cases_are_not_hollow():
    total = np.zeros(4, np.int64)
    for case in CASES:
        spec, rows, st, queries = random_case(case)
        per = np.array([census_of(case[1], st, spec, q) for q in queries])
        assert (per[:, :2].sum(axis=0) > 0).all() and per[:, 3].sum() > 0, (case, per.tolist())     # in every case
        total += per.sum(axis=0)
    print("census (unreachable passable, no source, deeper than H + W, impassable source):", total.tolist())
    assert (total >= [100, 50, 5, 100]).all(), total.tolist()                # (with SEED0 = 100: 569, 271, 7, 459)


class DistSet:
    """`rows` states in the two members a distance query reads.  guard=True: each member is a view one row into an allocation with
    a row of other bytes on either side; guard=False: the members ARE their allocations."""

    def __init__(self, spec, rows, states, guard=True, seed=0):
        r = np.random.default_rng(seed)
        self.spec, self.rows, self.cb, self.host = spec, rows, cell_bytes_of(spec), states
        self.dev, self.keep = {}, []
        for m, arr in states.items():
            arr = arr.view(np.int16) if arr.dtype == np.uint16 else arr      # (the 16-bit cells: torch's int16)
            if guard:
                pad = r.integers(0, 256, size=(1,) + arr.shape[1:]).astype(arr.dtype)
                full = torch.from_numpy(np.concatenate([pad, arr, pad])).to(DEV)
                self.keep.append(full)
                self.dev[m] = full[1:rows + 1]
            else:
                self.dev[m] = torch.from_numpy(np.ascontiguousarray(arr)).to(DEV)


def dist_both(be, st, n, idx, q, ctx, outputs="fa", bad=True, lead=1):
    """one mgx_distance and the model's answer: the outputs (each starts `lead` int16 into a buffer of 0x7777), the guard words around
    them, and the bad words.  outputs: "f" the field, "a" agent_dist, "fa" both in one launch.  Returns the model's (field, agent_dist)
    of the n output rows (rows of a bad index: as the kernel leaves them)."""
    sp = st.spec
    A, HW = sp.num_agents, sp.width * sp.height
    idx = None if idx is None else np.asarray(idx, dtype=np.int64)
    src = np.arange(n) if idx is None else idx
    ok = (src >= 0) & (src < st.rows)
    safe = np.where(ok, src, 0)
    pts = q.get("points")
    pts = None if pts is None else np.ascontiguousarray(pts[:n])
    qm = dict(q, points=pts)
    d, ad = model_distance(st.cb, st.host["cells"][safe], st.host["agents"][safe], sp, **qm)
    d, ad = d.reshape(n, HW).copy(), ad.copy()
    d[~ok], ad[~ok] = FILL, FILL
    bufs = {}
    for name, per in (("f", HW), ("a", A)):
        if name in outputs:
            full = torch.full((lead + n * per + 8,), FILL, dtype=torch.int16, device=DEV)
            bufs[name] = (full, full[lead:lead + n * per].view((n, sp.height, sp.width) if name == "f" else (n, A)), per)
    bad_d = torch.tensor([0, INT32_MAX], dtype=torch.int32, device=DEV) if bad else None
    query = dict(type_mask=q.get("type_mask", 0), colour_mask=q.get("colour_mask", 0xFF), agent_mask=q.get("agent_mask", 0), flags=q.get("flags", 0),
                 points=None if pts is None else torch.from_numpy(pts).to(DEV))
    be.distance(n, st.dev, st.rows, None if idx is None else torch.from_numpy(idx).to(DEV), query,
                bufs["f"][1] if "f" in bufs else None, bufs["a"][1] if "a" in bufs else None, bad_d)
    for name, want in (("f", d), ("a", ad)):
        if name in bufs:
            full, _, per = bufs[name]
            got = full.cpu().numpy()
            assert (got[:lead] == FILL).all() and (got[lead + n * per:] == FILL).all(), f"{ctx}: a guard word of '{name}' was written"
            body = got[lead:lead + n * per].reshape(n, per)
            wrong = np.argwhere(body != want)
            assert not len(wrong), f"{ctx} '{name}': {len(wrong)} wrong, first (row, cell) {wrong[0].tolist()}: {body[tuple(wrong[0])]} for {want[tuple(wrong[0])]}"
    if bad:
        first = int(np.flatnonzero(~ok)[0]) if (~ok).any() else INT32_MAX
        assert bad_d.cpu().tolist() == [int((~ok).sum()), first], ctx + ": bad"
    return d.reshape(n, sp.height, sp.width), ad


@gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{s}_{FORMAT[cb]}_A{A}" for s, cb, A in CASES])
def test_kernel_equals_the_model(case):
    shape, cb, A = case
    spec, rows, states, queries = random_case(case)
    H, W = SHAPES[shape]
    group, per = geometry(W, H, rows)[:2]
    assert rows == 2 * per + 1 and group == {3: 4, 5: 8, 7: 8, 8: 8, 16: 16, 17: 32, 33: 64, 64: 64}[H]
    be, st = backend(spec), DistSet(spec, rows, states, seed=CASES.index(case))
    r = np.random.default_rng(CASES.index(case))
    for k, n in enumerate((1, 2 * per - 1, 2 * per + 1)):
        for j, q in enumerate(queries):
            ctx = f"{shape} {FORMAT[cb]} A={A} n={n} query {j}"
            dist_both(be, st, n, None, q, ctx + " identity", outputs=("fa", "f", "a")[(k + j) % 3], lead=(k + j) % 2)
            dist_both(be, st, n, r.integers(0, rows, size=n), q, ctx + " repeats", outputs=("a", "fa", "f")[(k + j) % 3], bad=j != 1)
    n = 2 * per + 1
    ids = r.integers(0, rows, size=n)
    ids[0], ids[n // 2], ids[n - 1] = -1, rows, -1                              # == rows, and negative: counted, their rows left alone
    dist_both(be, st, n, ids, queries[0], f"{shape} {FORMAT[cb]} A={A} out of range")
    ids[n // 2], ids[n - 1] = 2 ** 40, -2 ** 40
    dist_both(be, st, n, ids, queries[1], f"{shape} {FORMAT[cb]} A={A} far out of range, nobody counts", bad=False, lead=3)


def open_states(rows, W, H, A, cb, where=(1, 1)):
    g = np.zeros((rows, H, W, 3), np.uint8)
    g[..., 0] = EMPTY
    return {"cells": pack(cb, g), "agents": agents_at([where] * A, rows)}


@gpu
@pytest.mark.parametrize("shape", ["3x3_group4", "8x8", "16x16", "17x9_group32"])
def test_neighbouring_envs_of_a_wavefront_do_not_leak(shape):
    """(a) every env is wide open, without a wall ring; only envs 1 mod 3 have sources -- the four corners: their top and bottom
    rows -- and the envs on either side of them, whose rows sit in the neighbouring lanes, must stay all -1"""
    H, W = SHAPES[shape]
    for cb in (2, 1, 3):
        rows = 2 * geometry(W, H, 1)[1] + 1
        spec = spec_for(W, H, 2, cb)
        st = DistSet(spec, rows, open_states(rows, W, H, 2, cb))
        pts = np.full((rows, 4, 2), -1, np.int16)
        pts[1::3] = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
        d, ad = dist_both(backend(spec), st, rows, None, dict(points=pts), f"leak {shape} {FORMAT[cb]}")
        assert (d[0::3] == -1).all() and (d[2::3] == -1).all() and (ad[0::3] == -1).all()
        assert (d[1::3] >= 0).all() and d[1::3].max() == (W - 1) // 2 + (H - 1) // 2 and d[1, 0, 0] == 0 and d[1, H - 1, W - 1] == 0


@gpu
def test_the_first_and_the_last_column():
    """(b) W == 64 with sources in columns 0 and 63 -- the horizontal shifts must not wrap --, and W < 64 with open cells in the last
    column -- the shift must not carry the flood into column W"""
    for H, W in ((5, 64), (64, 64), (7, 6), (64, 3), (33, 64)):
        for cb in (2, 1, 3):
            spec = spec_for(W, H, 1, cb)
            rows = 3
            states = open_states(rows, W, H, 1, cb, where=(W - 1, H - 1))
            g = np.zeros((rows, H, W, 3), np.uint8)
            g[..., 0] = EMPTY
            g[1, :, 1:W - 1] = (WALL, 5, 0)                                    # env 1: two open columns, joined nowhere
            g[2, :, 0], g[2, :, W - 1] = (GOAL, 1, 0), (GOAL, 1, 0)            # env 2: the sources ARE the two columns
            states["cells"] = pack(cb, g)
            st = DistSet(spec, rows, states)
            pts = np.array([[(0, H // 2), (W - 1, H // 2)]] * rows, np.int16)
            d, _ = dist_both(backend(spec), st, rows, None, dict(points=pts), f"columns {H}x{W} {FORMAT[cb]} points")
            assert d[0, H // 2, 0] == 0 and d[0, H // 2, W - 1] == 0 and d[0].max() == (W - 1) // 2 + max(H // 2, H - 1 - H // 2)
            assert (d[1, :, 0] >= 0).all() and (d[1, :, W - 1] >= 0).all() and (d[1, :, 1:W - 1] == -1).all()
            one = np.array([[(W - 1, 0)]] * rows, np.int16)
            d, _ = dist_both(backend(spec), st, rows, None, dict(points=one), f"columns {H}x{W} {FORMAT[cb]} one point")
            assert d[0, H - 1, 0] == W - 1 + H - 1 and (d[1, :, 0] == -1).all() and d[1, H - 1, W - 1] == H - 1
            d, _ = dist_both(backend(spec), st, rows, None, dict(type_mask=1 << GOAL), f"columns {H}x{W} {FORMAT[cb]} types")
            assert (d[2, :, 0] == 0).all() and (d[2, :, W - 1] == 0).all() and d[2].max() == (W - 1) // 2 and (d[:2] == -1).all()


def serpentine(H, W):
    """rows 0, 2, ... open, joined alternately at their ends; no wall ring.  (grid [H,W,3], the far end (x, y), its distance from (0, 0))"""
    g = np.zeros((H, W, 3), np.uint8)
    g[...] = (WALL, 5, 0)
    g[0::2] = (EMPTY, 0, 0)
    for k, y in enumerate(range(1, H - 1, 2)):
        g[y, W - 1 if k % 2 == 0 else 0] = (EMPTY, 0, 0)
    lanes = (H + 1) // 2
    end = (W - 1 if lanes % 2 else 0, 2 * (lanes - 1))
    return g, end, lanes * (W - 1) + 2 * (lanes - 1)


@gpu
def test_envs_of_very_different_depth_in_one_wavefront():
    """(c) 8x8, eight envs to the wavefront: a serpentine (34 levels), an open grid (14), no source at all, a walled-in source (0), ..."""
    H = W = 8
    snake, end, far = serpentine(H, W)
    assert far == 4 * 7 + 6 == 34 and end == (0, 6)
    for cb in (2, 1, 3):
        rows = 17
        g = np.zeros((rows, H, W, 3), np.uint8)
        g[..., 0] = EMPTY
        g[0::4] = snake
        g[3::4] = (WALL, 5, 0)
        states = {"cells": pack(cb, g), "agents": agents_at([end, (7, 7)], rows)}
        pts = np.zeros((rows, 1, 2), np.int16)
        pts[2::4] = (-1, -1)
        spec = spec_for(W, H, 2, cb)
        d, ad = dist_both(backend(spec), DistSet(spec, rows, states), rows, None, dict(points=pts), f"depths {FORMAT[cb]}")
        assert ad[0::4, 0].tolist() == [far] * 5 and ad[1::4, 1].tolist() == [14] * 4 and (d[2::4] == -1).all()
        assert (d[3::4].reshape(4, -1).max(axis=1) == 0).all() and (d[3::4, 0, 0] == 0).all()


@gpu
@pytest.mark.parametrize("cb", [2, 1, 3])
def test_the_64x64_serpentine_uses_the_twelfth_plane(cb):
    """(d) 2078 levels = 32 * 64 + 31 - 1 >= 2048.  No wall ring: through the backend, which `load_state` does not guard."""
    H = W = 64
    snake, end, far = serpentine(H, W)
    assert far == 2078 and end == (0, 62)
    spec = spec_for(W, H, 1, cb)
    g = np.stack([snake, np.full_like(snake, 0), snake])
    g[1, ..., 0], g[1, ..., 1] = WALL, 5
    states = {"cells": pack(cb, g), "agents": agents_at([end], 3)}
    st = DistSet(spec, 3, states)
    assert model_distance(cb, states["cells"], states["agents"], spec, points=np.zeros((3, 1, 2), np.int16))[1][0, 0] == 2078
    d, ad = dist_both(backend(spec), st, 3, None, dict(points=np.zeros((3, 1, 2), np.int16)), f"serpentine {FORMAT[cb]}")
    assert ad[:, 0].tolist() == [2078, -1, 2078] and d[0].max() == 2078 and d[0, 62, 0] == 2078 and d[1].max() == 0     # (env 1 is all wall: its source, walled in)
    d, ad = dist_both(backend(spec), st, 3, None, dict(agent_mask=1), f"serpentine {FORMAT[cb]} from the far end", outputs="f")
    assert d[0, 0, 0] == 2078 and d[2, 62, 0] == 0


@gpu
def test_every_flag_alone_and_all_together():
    """(e) on grids where each flag matters: the census below says so"""
    W, H, A = 16, 16, 4
    for cb in (2, 1, 3):
        states = random_grids(np.random.default_rng(50 + cb), 9, W, H, A, cb, wall=0.15)
        spec = spec_for(W, H, A, cb)
        be, st = backend(spec), DistSet(spec, 9, states)
        base = None
        for flags in (0, THROUGH_CLOSED, THROUGH_LOCKED, THROUGH_OBJECTS, AVOID_LAVA, 15):
            d, _ = dist_both(be, st, 9, None, dict(type_mask=1 << GOAL, flags=flags), f"flags {flags} {FORMAT[cb]}")
            if base is None:
                base = d
            else:
                assert (d != base).any(), f"flag {flags} changes nothing on these grids"
                assert flags != AVOID_LAVA or ((d >= 0) <= (base >= 0)).all()
                assert flags not in (THROUGH_CLOSED, THROUGH_LOCKED, THROUGH_OBJECTS) or ((base >= 0) <= (d >= 0)).all()


@gpu
def test_every_source_selector_alone_and_mixed():
    """(f) types; types narrowed by colour; agents -- one of them outside the grid: ignored as a source, answered -1 --; points, some
    outside the grid; and all of them at once"""
    W, H, A = 9, 17, 4
    for cb in (2, 1, 3):
        r = np.random.default_rng(60 + cb)
        rows = 5
        states = random_grids(r, rows, W, H, A, cb, wall=0.2)
        states["agents"][0, 1, 2:4] = (W, 3)                                  # beside the grid ...
        states["agents"][1, 0, 2:4] = (2, H)                                  # ... below it ...
        states["agents"][2, 2, 2:4] = (255, 255)                              # ... and far away
        states["agents"][3, 3, 2:4] = (64 + 2, 3)                             # (x & 63 would be a column of the grid)
        pts = np.array([[(1, 1), (W, 0), (-1, 5), (W - 1, H - 1), (3, -1), (0, H)]] * rows, np.int16)
        spec = spec_for(W, H, A, cb)
        be, st = backend(spec), DistSet(spec, rows, states)
        out = {}
        for name, q in (("types", dict(type_mask=1 << DOOR | 1 << LAVA)), ("colours", dict(type_mask=1 << DOOR | 1 << LAVA, colour_mask=0b101)),
                        ("agents", dict(agent_mask=0b1111)), ("agent 1", dict(agent_mask=0b10)), ("points", dict(points=pts)),
                        ("no agent", dict(agent_mask=0xFFFFFFF0)),
                        ("mixed", dict(type_mask=1 << DOOR | 1 << LAVA, colour_mask=0b101, agent_mask=0b0110, points=pts, flags=THROUGH_OBJECTS))):
            out[name] = dist_both(be, st, rows, None, q, f"selector {name} {FORMAT[cb]}")
        assert out["agents"][1][0].tolist()[1] == -1 and out["agents"][1][1, 0] == -1 and out["agents"][1][2, 2] == -1 and out["agents"][1][3, 3] == -1
        assert (out["agents"][1][0, [0, 2, 3]] == 0).all() and (out["agent 1"][0][0] == -1).all()     # (its only source lies outside)
        assert (out["no agent"][0] == -1).all()
        assert ((out["colours"][0] == 0) <= (out["types"][0] == 0)).all() and (out["colours"][0] == 0).sum() < (out["types"][0] == 0).sum()
        assert (out["points"][0][:, 1, 1] == 0).all() and (out["points"][0][:, H - 1, W - 1] == 0).all() and (out["points"][0] == 0).sum() == 2 * rows


# ---- real envs ---------------------------------------------------------------------------------------------------------------------

EMPTY8 = EnvSpec(8, 8, 2, 7, max_steps=8, allow_agent_overlap=False)
BUP = EnvSpec(16, 16, 4, 7, max_steps=1024, joint_reward=True, allow_agent_overlap=False, env_kind="blockedunlockpickup")


@gpu
def test_blockedunlockpickup_envs_and_their_snapshot_have_the_models_distances():
    """(g), (h): real envs; a snapshot's rows; repeated and bad indices; out= reuse"""
    B, A = 64, BUP.num_agents
    st = util.random_state(BUP, B, seed=5, box_contents_p=0.6)
    env = BatchedMultiGridEnv(BUP, B, DEV)
    env.load_state(st["grid"], st["agents"], st["rng"], st["target"], st["step_count"])
    q = dict(types=[Type.key, Type.goal], through=("closed", "objects"))
    want_f, want_a = model_distance(3, st["grid"], st["agents"], BUP, type_mask=1 << KEY | 1 << GOAL, flags=THROUGH_CLOSED | THROUGH_OBJECTS)
    plain_a = model_distance(3, st["grid"], st["agents"], BUP, type_mask=1 << KEY | 1 << GOAL)[1]
    assert (want_a >= 0).all() and len(np.unique(want_a)) > 8 and want_f.max() > 8 and (want_f == -1).any() and (plain_a != want_a).any()
    field, dist = env.distance_field(**q), env.agent_distance(**q)
    assert field.dtype is torch.int16 and field.cpu().numpy().tolist() == want_f.tolist() and dist.cpu().numpy().tolist() == want_a.tolist()
    assert env.agent_distance(types=[Type.key, Type.goal]).cpu().numpy().tolist() == plain_a.tolist()
    snap = env.snapshot()
    for t in range(3):
        env.step(torch.from_numpy(util.random_actions(B, A, seed=t, p_missing=0.0)).to(DEV))
    assert (env.agent_distance(**q) != dist).any()
    rows = torch.tensor([3, 3, B - 1, B, 0], device=DEV)                       # (one row out of range: left alone, and counted)
    out = torch.full((5, A), FILL, dtype=torch.int16, device=DEV)
    assert snap.agent_distance(rows, out=out, **q) is out
    assert out.cpu().tolist() == want_a[[3, 3, B - 1]].tolist() + [[FILL] * A, want_a[0].tolist()]
    with pytest.raises(ValueError, match=r"1 pair\(s\) named an env id or a snapshot row out of range.*first at pair 3"):
        env.check_errors()
    fout = torch.full((5, 16, 16), FILL, dtype=torch.int16, device=DEV)
    assert snap.distance_field(rows, out=fout, **q) is fout
    assert fout[[0, 1, 2, 4]].cpu().tolist() == want_f[[3, 3, B - 1, 0]].tolist() and (fout[3] == FILL).all()
    with pytest.raises(ValueError, match="out of range"):
        env.check_errors()
    pts = torch.tensor([[[1, 1]], [[2, 2]], [[14, 14]]], dtype=torch.int16, device=DEV)    # points go by OUTPUT row
    got = snap.distance_field(rows[:3], points=pts, out=fout[:3])
    assert got.cpu().tolist() == model_distance(3, st["grid"][[3, 3, B - 1]], st["agents"][[3, 3, B - 1]], BUP, points=pts.cpu().numpy())[0].tolist()
    env.restore(snap)
    assert torch.equal(env.agent_distance(out=dist.clone(), **q), dist) and torch.equal(env.distance_field(**q), field)
    env.check_errors()


@gpu
def test_a_step_and_its_distances_in_one_graph():
    """(i) one branch: the step, then the query behind it on the same stream; replayed after steps that change the state"""
    B, A = 130, 2
    env = make_env("pool", B=B, spec=EMPTY8, dev=DEV)
    twin = make_env("pool", B=B, spec=EMPTY8, backend=DistOracle(EMPTY8))
    acts = actions_for(B, A, 5, 1)
    buf = acts[0].to(DEV).clone()
    dist = torch.zeros((B, A), dtype=torch.int16, device=DEV)
    field = torch.zeros((B, 8, 8), dtype=torch.int16, device=DEV)
    cur = torch.cuda.current_stream(torch.device(DEV))
    side, graph = torch.cuda.Stream(torch.device(DEV)), torch.cuda.CUDAGraph()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        env.step(buf, auto_reset=True); env.agent_distance(types=[Type.goal], out=dist); env.distance_field(agents=[0], out=field)
        with torch.cuda.graph(graph, stream=side):                            # (everything bound and allocated before the capture)
            env.step(buf, auto_reset=True)
            env.agent_distance(types=[Type.goal], out=dist)
            env.distance_field(agents=[0], out=field)
    cur.wait_stream(side)
    twin.step(acts[0], auto_reset=True)
    assert dist.cpu().tolist() == twin.agent_distance(types=[Type.goal]).tolist()
    seen = set()
    for t in range(1, 4):                                                     # three replays, each another step
        buf.copy_(acts[t].to(DEV))
        dist.fill_(FILL); field.fill_(FILL)
        graph.replay()
        twin.step(acts[t], auto_reset=True)
        assert dist.cpu().tolist() == twin.agent_distance(types=[Type.goal]).tolist(), t
        assert field.cpu().tolist() == twin.distance_field(agents=[0]).tolist(), t
        assert env.agents.cpu().tolist() == twin.agents.tolist(), t
        seen |= set(dist.cpu().reshape(-1).tolist())
    assert len(seen) > 4
    env.check_errors()


@gpu
def test_c_abi_return_codes_on_the_device():
    """the header's order with real pointers: n == 0 launches nothing, a side of 65 is unsupported, and a plain call answers"""
    L = _lib.lib()
    W, H, A, rows = 5, 5, 2, 4
    g, _ = layouts.empty_layout(5, 1)
    cells = torch.from_numpy(layouts.pack_cells(np.stack([g] * rows)).view(np.int16)).to(DEV)
    agents = torch.from_numpy(agents_at([(1, 1), (2, 3)], rows)).to(DEV)
    field = torch.full((rows, H, W), FILL, dtype=torch.int16, device=DEV)
    dist = torch.full((rows, A), FILL, dtype=torch.int16, device=DEV)
    members = [n for n, _ in _lib.MgxEnvRows._fields_[:-1]]
    src = _lib.MgxEnvRows(*[{"cells": cells.data_ptr(), "agents": agents.data_ptr()}.get(m) for m in members], rows)
    q = _lib.MgxDistanceC(1 << GOAL, 0xFF, 0, 0, None, 0)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream

    def D(spec, n, q_=q, f=field.data_ptr(), a=dist.data_ptr()):
        return L.mgx_distance(C.byref(spec.to_c()), n, C.byref(src), None, C.byref(q_), f, a, None, stream)
    ok = EnvSpec(W, H, A, 3)
    assert D(ok, -1) == _lib.ERR_INVALID_ARGUMENT and D(ok, rows, _lib.MgxDistanceC(1, 0xFF, 0, 16, None, 0)) == _lib.ERR_INVALID_ARGUMENT
    assert D(ok, 0) == 0 and D(EnvSpec(65, 5, A, 3), 0) == 0                   # n == 0 comes first ...
    torch.cuda.synchronize()
    assert (field == FILL).all() and (dist == FILL).all()                      # ... and launches nothing
    assert D(ok, rows, f=None, a=None) == _lib.ERR_INVALID_ARGUMENT and D(ok, rows, f=field.data_ptr() + 1) == _lib.ERR_INVALID_ARGUMENT
    assert D(ok, rows, _lib.MgxDistanceC(0, 0xFF, 0, 0, None, 1)) == _lib.ERR_INVALID_ARGUMENT
    assert D(EnvSpec(65, 5, A, 3), rows) == _lib.ERR_UNSUPPORTED and D(EnvSpec(5, 65, A, 3), rows) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (field == FILL).all() and (dist == FILL).all()
    assert D(ok, rows) == 0
    torch.cuda.synchronize()
    want_f, want_a = model_distance(3, np.stack([g] * rows), agents.cpu().numpy(), ok, type_mask=1 << GOAL)
    assert field.cpu().tolist() == want_f.tolist() and dist.cpu().tolist() == want_a.tolist() == [[4, 1]] * rows
