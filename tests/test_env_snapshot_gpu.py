"""Snapshot, restore and fork on the GPU: env_copy_kernel (csrc/mgx_env_copy.hip) against the sequential NumPy model of
tests/test_env_snapshot.py, byte for byte -- first on synthetic state sets through the C ABI, at the smallest shapes that reach every
copy unit and both paths of the tile copy, whole ALLOCATIONS compared (every set is a view one row into a larger tensor, so a byte
outside the named rows shows up); then through BatchedMultiGridEnv.snapshot / restore / fork on small real envs, against a twin env
that is never restored and takes the same actions."""
import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec
from tests.test_env_snapshot import (CANDIDATES, INT32_MAX, NONE, OUTPUTS, SNAPSHOTS, TRIO, assert_same_run, make_env, model_env_copy,
                                     run, state_of)
from tests.test_episode_stats import actions_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

NULLABLE = ("aux", "marker", "episode", "gen_state", "trio")
#: (W, H, cell_bytes): tile bytes -> the copy unit (mgx_aux_geom.h: env_copy_unit) and the path of the tile copy
SHAPES = {
    "5x5_compact_25B_unit1": (5, 5, 1),
    "5x5_16bit_50B_unit2": (5, 5, 2),
    "6x5_16bit_60B_unit4": (6, 5, 2),
    "6x6_16bit_72B_unit8": (6, 6, 2),
    "8x8_16bit_128B_unit16": (8, 8, 2),
    "5x5_bytes_75B_unit1": (5, 5, 3),
    "64x64_compact_4096B_one_pair_per_wavefront": (64, 64, 1),
    "64x64_16bit_8192B_two_rounds_per_pair": (64, 64, 2),
}


def backend(spec):
    from multigrid_amd.ops import HipBackend
    return HipBackend(spec, torch.device(DEV))


class StateSet:
    """`rows` rows of every chosen member with recognisable (random) bytes, each a view one row into an allocation with a guard row
    on either side; `host` / `host_full`: the model's copy, `dev` / `dev_full`: the kernel's.  `cells_offset`: the cells start that
    many bytes into a flat byte buffer instead, so that their base address -- not the tile size -- bounds the copy unit."""

    def __init__(self, spec, rows, nullable, seed, cells_offset=None):
        A, r = spec.num_agents, np.random.default_rng(seed)
        shapes = {"cells": (np.int16 if spec.cell_bytes == 2 else np.uint8, tuple(spec.cells_shape(1)[1:])),
                  "agents": (np.uint8, (A, 8)), "rng": (np.int64, (4,)), "step_count": (np.int32, ())}
        if "aux" in nullable:
            shapes["aux"] = (np.uint8, (16,))
        if "marker" in nullable:
            shapes["marker"] = (np.int32, ())
        if "episode" in nullable:
            shapes["episode"] = (np.int32, ())
        if "gen_state" in nullable:
            shapes["gen_state"] = (np.int64, (6,))
        if "trio" in nullable:
            shapes.update(cur_return=(np.float64, (A,)), cur_length=(np.int32, ()), over=(np.uint8, ()))
        self.rows, self.host_full, self.dev_full, self.host, self.dev = rows, {}, {}, {}, {}
        for m, (dt, shape) in shapes.items():
            full = (rows + 2,) + shape
            nbytes = int(np.prod(full)) * np.dtype(dt).itemsize
            if m == "cur_return":
                arr = (r.integers(-8000, 8000, size=full) / 8.0).astype(np.float64)
            else:
                arr = r.integers(0, 256, size=nbytes, dtype=np.uint8).view(dt).reshape(full)
            if m == "cells" and cells_offset is not None:
                row = nbytes // (rows + 2)
                flat = np.concatenate([r.integers(0, 256, size=cells_offset, dtype=np.uint8), arr.view(np.uint8).reshape(-1),
                                       r.integers(0, 256, size=64, dtype=np.uint8)])
                self.host_full[m] = flat
                self.dev_full[m] = torch.from_numpy(flat).to(DEV)
                lo, hi = cells_offset + row, cells_offset + row * (rows + 1)
                self.host[m] = flat[lo:hi].view(dt).reshape((rows,) + shape)
                self.dev[m] = self.dev_full[m][lo:hi].view(torch.int16 if dt is np.int16 else torch.uint8).view((rows,) + shape)
                continue
            self.host_full[m] = arr
            self.dev_full[m] = torch.from_numpy(arr).to(DEV)
            self.host[m], self.dev[m] = arr[1:rows + 1], self.dev_full[m][1:rows + 1]

    def assert_equal(self, ctx):
        for m, t in self.dev_full.items():
            assert t.cpu().numpy().tobytes() == self.host_full[m].tobytes(), f"{ctx}: {m}"


def copy_both(be, n, src, src_idx, dst, dst_idx, stage_mode, marker_fill, ctx, tag_rows=True, bad=True):
    """one mgx_env_copy and the model's, compared over every allocation, the tags and the bad words"""
    as_dev = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)
    tag = tag_d = None
    if stage_mode != NONE and tag_rows:
        tag = np.random.default_rng(5).integers(-3, 50, size=(dst.rows, 4)).astype(np.int32)
        tag_d = torch.from_numpy(tag).to(DEV)
    bad_h = np.array([0, INT32_MAX], np.int32) if bad else None
    bad_d = torch.from_numpy(bad_h).to(DEV) if bad else None
    be.env_copy(n, src.dev, src.rows, as_dev(src_idx), dst.dev, dst.rows, as_dev(dst_idx), tag_d, stage_mode,
                marker_fill, bad_d)
    model_env_copy(n, src.host, src.rows, src_idx, dst.host, dst.rows, dst_idx, tag, stage_mode, marker_fill, bad_h)
    dst.assert_equal(ctx)
    src.assert_equal(ctx + " (source)")
    if tag is not None:
        assert tag_d.cpu().numpy().tolist() == tag.tolist(), ctx + ": tags"
    if bad:
        assert bad_d.cpu().numpy().tolist() == bad_h.tolist(), ctx + ": bad"
    return bad_h


def presence(k):
    """variant k of who carries what: over k = 0..3 every nullable member is seen in both sets, in the source only, in the
    destination only and in neither"""
    src, dst = [], []
    for j, m in enumerate(NULLABLE):
        combo = (k + j) % 4
        if combo & 1:
            src.append(m)
        if combo >> 1:
            dst.append(m)
    return src, dst


@pytest.mark.parametrize("A", [1, 2, 3, 32])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_equals_the_model(shape, A):
    W, H, cb = SHAPES[shape]
    spec = EnvSpec(W, H, A, 3, cell_bytes=cb)
    be = backend(spec)
    B, r = 130, np.random.default_rng(A * 100 + W + cb)
    for k in range(4):
        src_m, dst_m = presence(k)
        ctx = f"{shape} A={A} variant {k}"
        # a snapshot: n of the B rows into a set of n rows
        n = (0, 1, 5, 130)[k]
        src, dst = StateSet(spec, B, src_m, 10 + k), StateSet(spec, max(n, 1), dst_m, 20 + k)
        ids = None if k == 3 else r.permutation(B)[:n]
        copy_both(be, n, src, ids, dst, None, NONE, k >> 1, ctx + f" snapshot n={n}", bad=k != 2)
        # a restore: 200 pairs with repeated rows into a set of 256
        src, dst = StateSet(spec, B, src_m, 30 + k), StateSet(spec, 256, dst_m, 40 + k)
        rows, ids = r.integers(0, B, size=200), r.permutation(256)[:200]
        assert len(np.unique(rows)) < 200
        copy_both(be, 200, src, rows, dst, ids, (CANDIDATES, SNAPSHOTS)[k % 2], k >> 1, ctx + " restore", tag_rows=k != 1)
    # identity on both sides, into a larger set: the first B rows
    src, dst = StateSet(spec, B, NULLABLE, 50), StateSet(spec, 256, NULLABLE, 51)
    copy_both(be, B, src, None, dst, None, SNAPSHOTS, 0, f"{shape} A={A} identity")
    assert dst.host["marker"][:B].tolist() == src.host["marker"].tolist()


@pytest.mark.parametrize("offset,unit", [(8, 8), (4, 4), (2, 2), (16, 16)])
def test_the_copy_unit_follows_the_base_address(offset, unit):
    """8x8 16-bit cells are 128-byte tiles: by size they move as 16-byte vectors.  Cells that start `offset` bytes into their
    allocation bound the unit by ADDRESS (the source's, the destination's, or both)."""
    spec = EnvSpec(8, 8, 2, 3)
    be = backend(spec)
    for where in ("src", "dst", "both"):
        src = StateSet(spec, 130, NULLABLE, 60, cells_offset=offset if where != "dst" else None)
        dst = StateSet(spec, 256, NULLABLE, 61, cells_offset=offset if where != "src" else None)
        addr = src.dev["cells"].data_ptr() | dst.dev["cells"].data_ptr()
        assert min(addr & -addr, 16) == unit                                  # the lowest set bit of either base
        r = np.random.default_rng(offset)
        copy_both(be, 200, src, r.integers(0, 130, size=200), dst, r.permutation(256)[:200], CANDIDATES, 0, f"offset {offset} {where}")


def test_bad_indices_are_skipped_whole_and_counted():
    spec = EnvSpec(6, 6, 3, 3)
    be = backend(spec)
    src, dst = StateSet(spec, 130, NULLABLE, 70), StateSet(spec, 256, NULLABLE, 71)
    r = np.random.default_rng(7)
    rows, ids = r.integers(0, 130, size=200), r.permutation(256)[:200]
    rows[17] = -1                  # negative
    rows[101] = 130                # == rows of the source
    ids[150] = 2 ** 40             # far beyond
    ids[199] = 256                 # == rows of the destination
    bad = copy_both(be, 200, src, rows, dst, ids, SNAPSHOTS, 0, "bad indices")
    assert bad.tolist() == [4, 17]
    # three, the first of them late; `bad` NULL: skipped silently
    rows, ids = r.integers(0, 130, size=200), r.permutation(256)[:200]
    rows[190], ids[195], ids[199] = -3, 256, 2 ** 40                       # negative, equal to `rows`, far beyond
    bad = copy_both(be, 200, src, rows, dst, ids, CANDIDATES, 1, "bad indices late")
    assert bad.tolist() == [3, 190]
    copy_both(be, 200, src, rows, dst, ids, CANDIDATES, 0, "bad indices, nobody counts", bad=False)


# ---- real envs ---------------------------------------------------------------------------------------------------------------------

EMPTY8 = EnvSpec(8, 8, 2, 7, max_steps=8)
BUP4 = EnvSpec(7, 4, 2, 7, max_steps=8, joint_reward=True, env_kind="blockedunlockpickup")


def real_env(case, B=130):
    if case == "bup4_candidates":
        env = BatchedMultiGridEnv(BUP4, B, DEV)
        env.set_layout_generator("blockedunlockpickup", layout_seed=5, room_size=4, staged="candidates")
        env.reset(seed=3)
        assert env._gen["stage"]["candidates"] == 2
        return env
    return make_env(case[len("empty8_"):], B=B, spec=EMPTY8, dev=DEV)


CASES = ["empty8_plain", "empty8_pool", "empty8_gen", "empty8_gen_candidates", "empty8_gen_between", "bup4_candidates"]


@pytest.mark.parametrize("case", CASES)
def test_a_restored_batch_continues_as_its_never_restored_twin(case):
    B = 130
    env, twin = real_env(case, B), real_env(case, B)
    sp, A, ar = env.spec, env.spec.num_agents, case != "empty8_plain"
    T = 2 * sp.max_steps + 3
    warm = actions_for(B, A, 3, 1).to(DEV)
    for t in range(3):
        env.step(warm[t], auto_reset=ar); twin.step(warm[t], auto_reset=ar)
    snap = env.snapshot()
    assert snap.rows == B
    other = actions_for(B, A, T, 2).to(DEV)                                   # the env goes its own way, through episode ends
    for t in range(T):
        env.step(other[t], auto_reset=ar)
    assert state_of(env)["agents"].tobytes() != state_of(twin)["agents"].tobytes()
    if ar:
        assert (env.episode >= 3).all()
    env.restore(snap)
    for k, v in state_of(twin).items():
        assert state_of(env)[k].tobytes() == v.tobytes(), k
    acts = actions_for(B, A, T, 3).to(DEV)
    assert_same_run(run(env, acts, ar), run(twin, acts, ar), case)
    if ar:                                            # (the counter came back with the rows: the first start and two more ends since)
        assert (env.episode >= 3).all() and torch.equal(env.episode, twin.episode)
    env.check_errors()


@pytest.mark.parametrize("case", ["empty8_pool", "empty8_gen", "bup4_candidates"])
def test_forks_run_as_their_sources_do_in_the_twin(case):
    B = 130
    env, twin = real_env(case, B), real_env(case, B)
    sp, A = env.spec, env.spec.num_agents
    T = 2 * sp.max_steps + 3
    warm = actions_for(B, A, 3, 1).to(DEV)
    for t in range(3):
        env.step(warm[t], auto_reset=True); twin.step(warm[t], auto_reset=True)
    r = np.random.default_rng(0)
    sources = np.array([5, 64, 129])
    dst = np.sort(r.permutation(B)[:100])
    which = r.integers(0, 3, size=100)
    assert set(sources) & set(dst), "a destination that is also a source hands on its old state"
    env.fork(torch.from_numpy(sources[which]).to(DEV), torch.from_numpy(dst).to(DEV), check=True)
    of = np.arange(B)                                                         # env b runs as env of[b] of the twin
    of[dst] = sources[which]
    now, was = state_of(env), state_of(twin)
    for k in was:
        assert now[k].tobytes() == was[k][of].tobytes(), k
    acts_twin = actions_for(B, A, T, 3)
    acts = acts_twin[:, torch.from_numpy(of)].contiguous()
    (steps, _), (steps_twin, _) = run(env, acts.to(DEV), True), run(twin, acts_twin.to(DEV), True)
    kept = np.setdiff1d(np.arange(B), dst)
    for t in range(T):
        for k in OUTPUTS + ("was_reset",):
            assert steps[t][k][kept].tobytes() == steps_twin[t][k][kept].tobytes(), (t, k)
    for j, s in enumerate(sources):
        group = dst[which == j]
        upto = T
        if case == "empty8_pool":                                            # up to the first restart: from there the slot's own layouts
            upto = min(t for t in range(T) if steps_twin[t]["was_reset"][s])
            assert all(steps[upto]["was_reset"][group])
        for t in range(upto):
            for k in OUTPUTS:
                assert (steps[t][k][group] == steps_twin[t][k][s]).all(), (case, j, t, k)
    env.check_errors()


def test_the_running_episode_travels_with_a_restore():
    B = 130
    env, twin = real_env("empty8_pool", B), real_env("empty8_pool", B)
    A, T = 2, 2 * EMPTY8.max_steps + 3
    stats, tstats = env.track_episodes(), twin.track_episodes()
    warm = actions_for(B, A, 5, 1).to(DEV)
    for t in range(5):
        env.step(warm[t], auto_reset=True); twin.step(warm[t], auto_reset=True)
    snap = env.snapshot()
    assert set(TRIO) <= set(snap.tensors)
    other = actions_for(B, A, T, 2).to(DEV)
    for t in range(T):
        env.step(other[t], auto_reset=True)
    totals = {n: t.clone() for n, t in stats.tensors.items() if n not in TRIO}
    t_totals = {n: t.clone() for n, t in tstats.tensors.items() if n not in TRIO}
    env.restore(snap)
    for n, t in stats.tensors.items():
        assert torch.equal(t, tstats.tensors[n] if n in TRIO else totals[n]), n
    acts = actions_for(B, A, T, 3).to(DEV)
    assert_same_run(run(env, acts, True), run(twin, acts, True))
    for n in TRIO:
        assert torch.equal(stats.tensors[n], tstats.tensors[n]), n
    for n in ("sum_length", "counts"):                                        # the same episodes were closed since
        assert torch.equal(stats.tensors[n] - totals[n], tstats.tensors[n] - t_totals[n]), n
    assert int((tstats.counts[:, 0] - t_totals["counts"][:, 0]).min()) >= 2 and not stats.counts[:, 3].any()


def test_restore_and_step_in_one_graph():
    B = 130
    env, twin = real_env("empty8_pool", B), real_env("empty8_pool", B)
    acts = actions_for(B, 2, 8, 1).to(DEV)
    for t in range(3):
        env.step(acts[t], auto_reset=True); twin.step(acts[t], auto_reset=True)
    snap = env.snapshot()
    assert env._mark["armed"], "the steps of this env keep the layout marker"
    twin.step(acts[3], auto_reset=True)
    want = {k: getattr(twin, k).clone() for k in OUTPUTS}
    want_state = state_of(twin)
    cur = torch.cuda.current_stream(torch.device(DEV))
    side, graph = torch.cuda.Stream(torch.device(DEV)), torch.cuda.CUDAGraph()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        env.restore(snap); env.step(acts[3], auto_reset=True)                 # (everything bound and allocated before the capture)
        with torch.cuda.graph(graph, stream=side):
            env.restore(snap)
            env.step(acts[3], auto_reset=True)
    cur.wait_stream(side)
    for replay in range(2):
        for t in range(4, 8):                                                 # the env moves on between the replays
            env.step(acts[t], auto_reset=True)
        graph.replay()
        for k in OUTPUTS:
            assert torch.equal(getattr(env, k), want[k]), (replay, k)
        for k, v in state_of(env).items():
            assert v.tobytes() == want_state[k].tobytes(), (replay, k)
    env.check_errors()
