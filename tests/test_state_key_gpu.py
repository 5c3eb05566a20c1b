"""State and observation keys on the GPU: state_key_kernel / obs_key_kernel (csrc/mgx_state_key.hip) against the NumPy statement of
the rule in tests/test_state_key.py, bit for bit -- first through the C ABI on synthetic state sets of random bytes (every member a
view one row into a larger allocation, the keys between two guard elements), at the smallest shapes that reach every load unit of
every cell format and every lane-group size of the launch geometry (csrc/mgx_aux_geom.h: state_key_geom; `geometry` restates it and
tests/test_state_key.py holds the restatement to the header); then through BatchedMultiGridEnv.state_key / obs_key and
EnvSnapshot.state_key on small real envs, against the model of an oracle-backed twin's state."""
import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec
from tests import util
from tests.test_env_snapshot import CopyOracle, make_env
from tests.test_episode_stats import actions_for, empty_pool
from tests.test_state_key import RNG, SALTS, STEP, cell_bytes_of, geometry, model_obs_key, model_state_key

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT32_MAX = 2 ** 31 - 1
GUARD = -0x0123456789ABCDEF

#: (W, H, cell_bytes): tile bytes -> the load unit (state_key_unit) and what a chunk is.  At the n of these cases (<= 130) a
#: wavefront owns one env and all 64 lanes share it; SMALL_GROUPS below reaches the other group sizes.
SHAPES = {
    "5x5_compact_25B_unit1_pieces_odd_cells": (5, 5, 1),
    "6x5_compact_30B_unit2_one_word_a_load": (6, 5, 1),
    "6x6_compact_36B_unit4": (6, 6, 1),
    "6x4_compact_24B_unit8": (6, 4, 1),
    "5x5_16bit_50B_unit2_pieces_odd_cells": (5, 5, 2),
    "6x5_16bit_60B_unit4_one_word_a_load": (6, 5, 2),
    "6x6_16bit_72B_unit8": (6, 6, 2),
    "8x8_16bit_128B_unit16": (8, 8, 2),
    "7x9_16bit_126B_unit2_odd_cells": (7, 9, 2),
    "5x5_bytes_75B_unit1_six_pieces": (5, 5, 3),
    "6x5_bytes_90B_unit2_three_pieces": (6, 5, 3),
    "64x64_compact_4096B_unit16_one_round": (64, 64, 1),
    "64x64_16bit_8192B_unit16_two_rounds": (64, 64, 2),
}


def backend(spec):
    from multigrid_amd.ops import HipBackend
    return HipBackend(spec, torch.device(DEV))


class KeySet:
    """`rows` rows of the five members a key reads, random bytes, each a view one row into an allocation with a guard row on either
    side.  `cells_offset`: the cells start that many bytes into a flat byte buffer instead, so that their base ADDRESS bounds the
    load unit."""

    def __init__(self, spec, rows, seed, cells_offset=None):
        A, r = spec.num_agents, np.random.default_rng(seed)
        cb = cell_bytes_of(spec)
        shapes = {"cells": (np.int16 if cb == 2 else np.uint8, tuple(spec.cells_shape(1)[1:])), "agents": (np.uint8, (A, 8)),
                  "rng": (np.int64, (4,)), "step_count": (np.int32, ()), "aux": (np.uint8, (16,))}
        self.rows, self.cb, self.host, self.dev, self.keep = rows, cb, {}, {}, []
        for m, (dt, shape) in shapes.items():
            full = (rows + 2,) + shape
            nbytes = int(np.prod(full)) * np.dtype(dt).itemsize
            arr = r.integers(0, 256, size=nbytes, dtype=np.uint8).view(dt).reshape(full)
            if m == "cells" and cells_offset is not None:
                row = nbytes // (rows + 2)
                flat = np.concatenate([r.integers(0, 256, size=cells_offset, dtype=np.uint8), arr.view(np.uint8).reshape(-1),
                                       r.integers(0, 256, size=64, dtype=np.uint8)])
                flat_d = torch.from_numpy(flat).to(DEV)
                lo, hi = cells_offset + row, cells_offset + row * (rows + 1)
                self.host[m] = flat[lo:hi].view(dt).reshape((rows,) + shape)
                self.dev[m] = flat_d[lo:hi].view(torch.int16 if dt is np.int16 else torch.uint8).view((rows,) + shape)
                self.keep.append(flat_d)
                continue
            full_d = torch.from_numpy(arr).to(DEV)
            self.keep.append(full_d)
            self.host[m], self.dev[m] = arr[1:rows + 1], full_d[1:rows + 1]

    def model(self, flags, salt, aux=True):
        h = self.host
        return model_state_key(self.cb, h["cells"], h["agents"], h["rng"], h["step_count"], h["aux"] if aux else None, flags,
                               salt).view(np.int64)


def key_both(be, st, n, idx, flags, salt, ctx, aux=True, bad=True):
    """one mgx_state_key and the model's keys: the keys, the guard elements around them and the bad words"""
    idx = None if idx is None else np.asarray(idx, dtype=np.int64)
    full = torch.full((n + 2,), GUARD, dtype=torch.int64, device=DEV)
    keys = full[1:n + 1]
    bad_d = torch.tensor([0, INT32_MAX], dtype=torch.int32, device=DEV) if bad else None
    rows = dict(st.dev) if aux else {m: t for m, t in st.dev.items() if m != "aux"}
    be.state_key(n, rows, st.rows, None if idx is None else torch.from_numpy(idx).to(DEV), flags, salt, keys, bad_d)
    per_row = st.model(flags, salt, aux)
    src = np.arange(n) if idx is None else idx
    ok = (src >= 0) & (src < st.rows)
    want = np.full(n + 2, GUARD, np.int64)
    want[1:n + 1][ok] = per_row[src[ok]]
    got = full.cpu().numpy()
    assert got[0] == GUARD and got[-1] == GUARD, ctx + ": a guard element was written"
    assert got.tolist() == want.tolist(), ctx
    if bad:
        first = int(np.flatnonzero(~ok)[0]) if (~ok).any() else INT32_MAX
        assert bad_d.cpu().tolist() == [int((~ok).sum()), first], ctx + ": bad"


@pytest.mark.parametrize("A", [1, 3, 32])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_equals_the_model(shape, A):
    W, H, cb = SHAPES[shape]
    spec = EnvSpec(W, H, A, 3, cell_bytes=cb)
    be = backend(spec)
    B, r = 130, np.random.default_rng(A * 100 + W * H + cb)
    st = KeySet(spec, B, 7 + A)
    unit = geometry(cb, W * H * cb, 1, st.dev["cells"].data_ptr())[2]
    assert f"unit{unit}_" in shape + "_" and geometry(cb, W * H * cb, B)[:2] == (1, 64)
    for k, (flags, salt) in enumerate([(0, SALTS[0]), (STEP, SALTS[1]), (RNG, SALTS[0]), (STEP | RNG, SALTS[1])]):
        ctx = f"{shape} A={A} flags={flags}"
        key_both(be, st, B, None, flags, salt, ctx + " identity", aux=k != 2)
        key_both(be, st, 67, r.permutation(B)[:67], flags, salt, ctx + " permutation")
        key_both(be, st, (1, 2, 63, 65)[k], r.integers(0, B, size=(1, 2, 63, 65)[k]), flags, salt, ctx + " repeats", bad=k % 2 == 0)
    ids = r.integers(0, B, size=67)
    ids[5], ids[66] = B, -1                                                   # == rows, and negative: counted, their keys left alone
    key_both(be, st, 67, ids, STEP, 1, f"{shape} A={A} out of range")
    ids[5], ids[66] = 2 ** 40, -2 ** 40
    key_both(be, st, 67, ids, 0, 1, f"{shape} A={A} far out of range, nobody counts", bad=False, aux=False)


def test_one_env_of_255_by_255_cells():
    """32 513 cell words: the index width"""
    spec = EnvSpec(255, 255, 3, 3)
    st = KeySet(spec, 2, 3)
    assert geometry(2, 255 * 255 * 2, 1)[2:] == (2, 4)
    key_both(backend(spec), st, 1, [1], STEP | RNG, SALTS[1], "255x255")
    key_both(backend(spec), st, 2, None, 0, 0, "255x255 both")


def _runs(tile_bytes):
    """the runs env_copy_geom's halving passes through on its way down from the tile's full run (1 excluded)"""
    out, run = [], max(1, min(64, 4096 // tile_bytes))
    while run > 1:
        out.append(run)
        run = (run + 1) // 2
    return out


#: a launch of n = 1024 * run - 1 envs gives a wavefront `run` envs and an env 64 / run lanes (rounded down to a power of two), and
#: leaves the last wavefront one env short of its run; 1024 * run + 1 adds a wavefront with a single env.  Byte triples pass through
#: runs that are no powers of two (54, 27, 14, 7): lanes of such a wavefront are left without an env.
SMALL_GROUPS = [(name, W, H, cb, run) for name, (W, H, cb) in (("5x5_compact", (5, 5, 1)), ("5x5_bytes", (5, 5, 3)), ("8x8_16bit", (8, 8, 2)))
                for run in _runs(W * H * cb)] + [("5x5_16bit", 5, 5, 2, 64)]


@pytest.mark.parametrize("name,W,H,cb,run", SMALL_GROUPS, ids=[f"{c[0]}_run{c[4]}_group{geometry(c[3], c[1] * c[2] * c[3], 1024 * c[4] - 1)[1]}"
                                                                for c in SMALL_GROUPS])
def test_lane_groups_of_every_size(name, W, H, cb, run):
    full_run = _runs(W * H * cb)[0]
    A = 32 if run == full_run else 3
    spec = EnvSpec(W, H, A, 3, cell_bytes=cb)
    be = backend(spec)
    rows = 1024 * run + 1
    st = KeySet(spec, rows, run)
    r = np.random.default_rng(run)
    for n in (1024 * run - 1, 1024 * run + 1) if run == full_run else (1024 * run - 1,):
        got_run, group = geometry(cb, W * H * cb, n)[:2]
        assert got_run == run and group * run <= 64 < 2 * group * run
        ids = r.integers(0, rows, size=n)
        ids[n // 2], ids[n - 1] = rows, -1
        key_both(be, st, n, ids, STEP | RNG, SALTS[1], f"{name} n={n}")
        key_both(be, st, n, None, 0, 0, f"{name} n={n} identity", aux=False)


@pytest.mark.parametrize("offset,cb,unit", [(8, 2, 8), (4, 2, 4), (2, 2, 2), (16, 2, 16), (1, 3, 1), (3, 3, 1), (2, 3, 2), (1, 1, 1), (2, 1, 2),
                                            (4, 1, 4), (8, 1, 8)])
def test_the_load_unit_follows_the_base_address(offset, cb, unit):
    """8x8 cells are 128 / 64 / 192-byte tiles: by size they are read as 16-byte vectors (byte triples: as 2-byte pieces).  Cells
    that start `offset` bytes into their allocation bound the unit by ADDRESS; byte triples at an odd offset are read byte by byte."""
    spec = EnvSpec(8, 8, 2, 3, cell_bytes=cb)
    st = KeySet(spec, 130, 60 + offset, cells_offset=offset)
    assert geometry(cb, 64 * cb, 130, st.dev["cells"].data_ptr())[2] == unit
    r = np.random.default_rng(offset)
    key_both(backend(spec), st, 130, r.integers(0, 130, size=130), STEP | RNG, SALTS[1], f"offset {offset} cb {cb}")
    big = KeySet(spec, 32 * 1024, 61 + offset, cells_offset=offset)          # ... and with several envs to a wavefront
    assert geometry(cb, 64 * cb, 32 * 1024 - 1)[1] < 64
    key_both(backend(spec), big, 32 * 1024 - 1, None, 0, 5, f"offset {offset} cb {cb}, groups")


@pytest.mark.parametrize("v", [3, 7, 15])
def test_obs_key_equals_the_model(v):
    """view rows of 27 / 147 / 675 bytes: a tail of 3 bytes each, dword-aligned only every fourth view"""
    assert 3 * v * v % 4 == 3
    spec = EnvSpec(16, 16, 2, v)
    be = backend(spec)
    r = np.random.default_rng(v)
    for n in (1, 65, 130):
        for lead in (1, 3):                                                  # (the views start `lead` bytes into their allocation)
            flat = torch.from_numpy(r.integers(0, 256, size=lead + n * 3 * v * v, dtype=np.uint8)).to(DEV)
            obs = flat[lead:].view(n, v, v, 3)
            dirs = torch.from_numpy(r.integers(0, 4, size=n, dtype=np.uint8)).to(DEV)
            full = torch.full((n + 2,), GUARD, dtype=torch.int64, device=DEV)
            be.obs_key(n, obs, dirs, SALTS[1], full[1:n + 1])
            want = [GUARD] + model_obs_key(obs.cpu().numpy(), dirs.cpu().numpy(), SALTS[1]).view(np.int64).tolist() + [GUARD]
            assert full.cpu().tolist() == want, (v, n, lead)
    # through the env, a rollout's [T, B, A, ...] outputs; the last view ends the allocation
    env = BatchedMultiGridEnv(spec, 5, DEV)
    obs = torch.from_numpy(r.integers(0, 256, size=(4, 5, 2, v, v, 3), dtype=np.uint8)).to(DEV)
    dirs = torch.from_numpy(r.integers(0, 4, size=(4, 5, 2), dtype=np.uint8)).to(DEV)
    keys = env.obs_key(obs, dirs)
    assert tuple(keys.shape) == (4, 5, 2) and keys.cpu().tolist() == model_obs_key(obs.cpu().numpy(), dirs.cpu().numpy()).view(np.int64).tolist()


# ---- real envs ---------------------------------------------------------------------------------------------------------------------

EMPTY8 = EnvSpec(8, 8, 2, 7, max_steps=8)
BUP = EnvSpec(16, 16, 4, 7, max_steps=1024, joint_reward=True, env_kind="blockedunlockpickup")


def oracle_keys(env, flags=0, salt=0):
    """the model on what an (oracle-backed) env shows"""
    return model_state_key(3, env.grid.cpu().numpy(), env.agents.cpu().numpy(), env.rng.cpu().numpy(), env.step_count.cpu().numpy(),
                           env.aux.cpu().numpy(), flags, salt).view(np.int64).tolist()


def test_empty_envs_have_the_keys_of_their_oracle_twin_at_every_step():
    B, T = 130, 2 * EMPTY8.max_steps + 3
    env = make_env("pool", B=B, spec=EMPTY8, dev=DEV)
    twin = make_env("pool", B=B, spec=EMPTY8, backend=CopyOracle(EMPTY8))
    acts = actions_for(B, 2, T, 2)
    seen = set()
    for t in range(T):
        for flags in (0, STEP | RNG):
            assert env.state_key(step_count=bool(flags & STEP), rng=bool(flags & RNG), salt=flags).cpu().tolist() == oracle_keys(twin, flags, flags), t
        seen |= set(env.state_key().cpu().tolist())
        env.step(acts[t].to(DEV), auto_reset=True)
        twin.step(acts[t], auto_reset=True)
        assert env.obs_key().cpu().tolist() == model_obs_key(twin.obs.numpy(), twin.dir.numpy()).view(np.int64).tolist(), t
    assert len(seen) > 100 and (env.episode >= 3).all()
    env.check_errors()


def test_blockedunlockpickup_envs_key_their_hook_state_and_box_contents():
    B, T = 64, 12
    st = util.random_state(BUP, B, seed=5, box_contents_p=0.6)
    assert ((st["grid"][..., 0] == 7) & (st["grid"][..., 2] > 3)).sum() > 20, "boxes that hold something"
    env = BatchedMultiGridEnv(BUP, B, DEV)
    twin = BatchedMultiGridEnv(BUP, B, "cpu", backend=util.OracleBackend(BUP))
    for e in (env, twin):
        e.load_state(st["grid"], st["agents"], st["rng"], st["target"], st["step_count"])
    for t in range(T):
        assert env.state_key(step_count=True, rng=True).cpu().tolist() == oracle_keys(twin, STEP | RNG), t
        act = torch.from_numpy(util.random_actions(B, BUP.num_agents, seed=t, p_missing=0.0))
        env.step(act.to(DEV))
        twin.step(act)
    keys = env.state_key()
    assert keys.cpu().tolist() == oracle_keys(twin)
    # the hook state and a box's content are part of the key
    env.aux[3, 1] ^= 1
    boxes = torch.nonzero((env.grid[..., 0] == 7) & (env.grid[..., 2] > 3))
    b, y, x = (int(v) for v in boxes[boxes[:, 0] != 3][0])
    env.cells[b, y, x] ^= 1 << 4                                             # the content's kind, bit 0
    changed = env.state_key() != keys
    assert changed.nonzero().flatten().tolist() == sorted([3, b])
    env.check_errors()


def test_sixteen_bit_and_compact_envs_in_step_have_equal_keys():
    B, T = 130, 8
    envs = []
    for cb in (2, 1):
        spec = EnvSpec(8, 8, 2, 7, max_steps=8, cell_bytes=cb)
        env = BatchedMultiGridEnv(spec, B, DEV)
        pg, pa = empty_pool(spec)
        env.load_state(pg[0], pa[0])
        env.seed(3)
        envs.append(env)
    acts = actions_for(B, 2, T, 2).to(DEV)
    for t in range(T):
        a, b = (e.state_key(step_count=True, rng=True, salt=SALTS[1]) for e in envs)
        assert torch.equal(a, b) and a.cpu().tolist() == oracle_keys(envs[1], STEP | RNG, SALTS[1]), t
        for e in envs:
            e.step(acts[t])


def test_forks_snapshots_and_restores_keep_their_keys():
    B = 130
    env = make_env("pool", B=B, spec=EMPTY8, dev=DEV)
    acts = actions_for(B, 2, 6, 4).to(DEV)
    for t in range(3):
        env.step(acts[t], auto_reset=True)
    before = env.state_key(step_count=True, rng=True)
    src, dst = torch.tensor([5, 5, 64, 129], device=DEV), torch.tensor([0, 7, 5, 100], device=DEV)
    env.fork(src, dst)
    after = env.state_key(step_count=True, rng=True)
    assert torch.equal(after[dst], before[src])
    keep = torch.from_numpy(np.setdiff1d(np.arange(B), dst.cpu().numpy())).to(DEV)
    assert torch.equal(after[keep], before[keep])
    assert len(torch.unique(after[torch.tensor([0, 7, 5], device=DEV)])) == 2   # the dedup: two forks of env 5, one of env 64
    snap = env.snapshot()
    at_snap = env.state_key(step_count=True)
    for t in range(3, 6):
        env.step(acts[t], auto_reset=True)
    assert (env.state_key(step_count=True) != at_snap).all()
    assert torch.equal(snap.state_key(step_count=True), at_snap)
    rows = torch.tensor([3, 3, 129, B, 0], device=DEV)                         # (one row out of range: left alone, and counted)
    out = torch.full((5,), GUARD, dtype=torch.int64, device=DEV)
    assert snap.state_key(rows, step_count=True, out=out) is out
    assert out.cpu().tolist() == at_snap[torch.tensor([3, 3, 129], device=DEV)].cpu().tolist() + [GUARD, int(at_snap[0])]
    with pytest.raises(ValueError, match=r"1 pair\(s\) named an env id or a snapshot row out of range.*first at pair 3"):
        env.check_errors()
    env.restore(snap)
    assert torch.equal(env.state_key(step_count=True), at_snap)
    env.check_errors()


def test_a_step_and_its_keys_in_one_graph():
    B = 130
    env, twin = make_env("pool", B=B, spec=EMPTY8, dev=DEV), make_env("pool", B=B, spec=EMPTY8, dev=DEV)
    acts = actions_for(B, 2, 8, 1).to(DEV)
    for t in range(3):
        env.step(acts[t], auto_reset=True); twin.step(acts[t], auto_reset=True)
    snap = env.snapshot()
    assert env._mark["armed"], "the steps of this env keep the layout marker"
    twin.step(acts[3], auto_reset=True)
    want = twin.state_key(step_count=True, rng=True)
    want_obs = twin.obs_key()
    keys = torch.zeros(B, dtype=torch.int64, device=DEV)
    obs_keys = torch.zeros((B, 2), dtype=torch.int64, device=DEV)
    cur = torch.cuda.current_stream(torch.device(DEV))
    side, graph = torch.cuda.Stream(torch.device(DEV)), torch.cuda.CUDAGraph()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        env.restore(snap); env.step(acts[3], auto_reset=True)                 # (everything bound and allocated before the capture)
        env.state_key(step_count=True, rng=True, out=keys); env.obs_key(out=obs_keys)
        with torch.cuda.graph(graph, stream=side):
            env.restore(snap)
            env.step(acts[3], auto_reset=True)
            env.state_key(step_count=True, rng=True, out=keys)
            env.obs_key(out=obs_keys)
    cur.wait_stream(side)
    for replay in range(2):
        for t in range(4, 8):                                                 # the env moves on between the replays
            env.step(acts[t], auto_reset=True)
        keys.zero_(); obs_keys.zero_()
        graph.replay()
        assert torch.equal(keys, want) and torch.equal(obs_keys, want_obs), replay
    assert env._mark["armed"]
    env.check_errors()


def test_the_example_dedups_its_forks():
    """examples/dedup_forks.py at C2's batch: 8 roots forked over 4096 envs, three levels of steps, forks and torch.unique"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "dedup_forks.py")
    mod_spec = importlib.util.spec_from_file_location("dedup_forks", path)
    mod = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(mod)
    out = mod.run("c2", roots=8, depth=3, device=DEV)
    levels = out["distinct_states_per_level"]
    assert out["batch"] == 4096 and len(levels) == 4 and levels[0] <= 8 < levels[1] < levels[2] <= levels[3] <= 4096

