"""The per-env layout marker of mgx_step_tracked (include/mgx.h): `grid_layout[b] = k >= 0` promises that env b's grid equals layout k
of the pool bit for bit, and the throughput family's launches skip the grid load of wavefronts whose envs all carry the same k.

  * tracked == untracked: two envs from one state and one action stream, one through mgx_step_tracked (step(auto_reset=True)), one
    through mgx_step_ex; every output and the whole state torch.equal after every one of 40 steps.  Empty-16x16 x 4 agents at 32 784
    envs (the smallest batch over 2048 wavefronts: the family that reads the marker) and at 64 / 100 envs (latency family, ragged
    last wavefront), max_steps = 8 so that restarts happen; the same with ONE layout that holds keys, doors and boxes (clean and
    dirty envs side by side in a wavefront that reads the marker) and with a pool of FOUR (consecutive envs on different layouts);
  * the invariant `grid_layout[b] >= 0  =>  cells[b] == pool[grid_layout[b]]` after every step of random actions on four layouts
    with keys, doors and boxes, with both transitions seen: clean -> dirty (a pickup / toggle) and dirty -> clean (a restart);
  * the fast path is really taken: with every env marked 0 and `_cells` overwritten behind the marker's back, a step observes the
    TRUE layout; with the marker at -1 the same step observes the overwritten grid;
  * everything that writes cells without keeping the marker takes the promise back (all -1) and the tracked steps after it equal the
    untracked ones; load_state_dict re-arms; split(2) shards hold slices of the marker; a captured graph of tracked steps equals
    eager ones.
The host-side bookkeeping alone (no GPU: the oracle backend ignores the marker) is test_marker_bookkeeping_on_the_oracle_backend."""
import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, layouts, rng as rnglib
from tests import util
from tests.test_reset_select import SelectOracle

DEV = "cuda:0"
STATE = ("_cells", "agents", "rng", "step_count", "aux", "episode")
OUT = ("obs", "dir", "reward", "terminated", "truncated", "was_reset")
THROUGHPUT = 32784           # 2049 wavefronts of 16 envs: the family that reads the marker, at this shape's full envs per wavefront
#                              (the other grid sizes that qualify, and the batches just outside: tests/test_marker_sizes_gpu.py)


def spec16(max_steps=8):
    return EnvSpec(16, 16, 4, 7, max_steps=max_steps)


def empty_pool():
    g, a = layouts.empty_layout(16, 4)
    return g[None].copy(), a[None].copy()


def object_pool(K, seed=11):
    """K walled 16x16 layouts with keys, balls, boxes and doors; agents alive, some carrying"""
    st = util.random_state(spec16(), K, seed, density=0.3, terminated_p=0.0)
    return st["grid"], st["agents"]


def make_env(spec, B, pool, device=DEV, backend=None, seed=3, rows=None):
    """B envs on the layouts of `pool` = (grids, agents[, auxs]), env b on layout b % K, with staggered step counts; rows=(lo, hi):
    only the envs lo .. hi-1 of that batch (a slice for the oracle: the kernels are data-parallel over envs)"""
    g, a = pool[0], pool[1]
    x = pool[2] if len(pool) > 2 else None
    lo, hi = rows if rows is not None else (0, B)
    b = np.arange(lo, hi)
    k = b % g.shape[0]                                     # the layout the pool gives env b in episode 0
    env = BatchedMultiGridEnv(spec, hi - lo, device, first_env=lo, backend=backend)
    env.load_state(g[k], a[k], rng=rnglib.synthetic_words(hi - lo, seed, lo), aux=None if x is None else x[k],
                   step_count=(b % spec.max_steps).astype(np.int32))
    env.set_layout_pool(g, a, x)
    return env


def untracked_stepper(env):
    """env's step with auto-reset through mgx_step_ex: the same launcher, bound without the marker"""
    f = env.backend.bind_step(env.batch, env._cells, env.agents, env.rng, env.step_count, env.aux if env.spec.env_kind != "empty" else None,
                              env.err, env.obs, env.dir, env.reward, env.terminated, env.truncated,
                              auto_reset=env._auto_reset_args(True, env.was_reset))
    assert not f.tracked
    return f


def actions(T, B, seed=5, A=4):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(0, 7, (T, B, A), dtype=torch.int8, device=DEV, generator=g)


def assert_same(e1, e2, ctx):
    for k in STATE + OUT:
        assert torch.equal(getattr(e1, k), getattr(e2, k)), f"{ctx}: {k} differs between the tracked and the untracked env"


def holds(env):
    """the invariant, on the device: grid_layout[b] >= 0 implies cells[b] == pool[grid_layout[b]]"""
    m = env._marker.long()
    same = (env._cells == env._pool[0][m.clamp(min=0)]).flatten(1).all(dim=1)
    return bool(((m < 0) | same).all())


POOLS = {"empty": empty_pool, "objects1": lambda: object_pool(1), "objects4": lambda: object_pool(4)}


@pytest.mark.gpu
@pytest.mark.parametrize("B,pool", [(THROUGHPUT, "empty"), (64, "empty"), (100, "empty"), (THROUGHPUT, "objects1"),
                                    (THROUGHPUT, "objects4"), (100, "objects4")])
def test_tracked_steps_equal_untracked_steps(B, pool):
    spec = spec16()
    e1, e2 = make_env(spec, B, POOLS[pool]()), make_env(spec, B, POOLS[pool]())
    step2 = untracked_stepper(e2)
    acts = actions(40, B)
    if pool != "objects4":
        assert int((e1._marker == 0).sum()) == B             # armed by the comparison with the one layout
    for t in range(40):
        e1.step(acts[t], auto_reset=True)
        step2(acts[t])
        assert_same(e1, e2, f"B={B} pool={pool} step {t}")
        assert holds(e1), f"B={B} pool={pool} step {t}: a marked env differs from its layout"
    assert e1._bound[(True, False)][2], "step(auto_reset=True) did not go through mgx_step_tracked"
    assert int(e1.episode.min()) >= 4                         # every env restarted several times
    if pool == "empty":
        assert int((e1._marker == 0).sum()) == B             # an Empty env never leaves its layout
    else:
        assert int((e1._marker < 0).sum()) > 0 and int((e1._marker >= 0).sum()) > 0
    if B == THROUGHPUT:
        assert e1.backend.launch_info(B)["envs_per_wavefront"] * 2048 < B      # more than 2048 wavefronts: the family that reads
    e1.check_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(256, 64), (THROUGHPUT, 24)])
def test_marked_envs_equal_their_layout_after_every_step(B, T):
    spec = spec16(max_steps=16 if B == 256 else 8)
    env = make_env(spec, B, object_pool(4))
    assert int((env._marker >= 0).sum()) == 0                  # four layouts: everything starts unknown, the restarts arm
    acts = actions(T, B, seed=9)
    to_dirty = to_clean = 0
    prev = env._marker.clone()
    for t in range(T):
        env.step(acts[t], auto_reset=True)
        assert holds(env), f"step {t}: a marked env differs from its layout"
        now = env._marker
        to_dirty += int(((prev >= 0) & (now < 0)).sum())
        to_clean += int(((prev < 0) & (now >= 0)).sum())
        # a restart names the layout the pool gives the env's new episode
        fresh = env.was_reset.bool() & (now >= 0)
        want = (torch.arange(B, device=DEV) + (env.episode.long() - 1) * 7919) % 4
        assert torch.equal(now[fresh].long(), want[fresh])
        prev = now.clone()
    assert to_dirty > 0, "no marked env was written by a pickup / toggle: the run does not test the commit's store"
    assert to_clean > 0, "no unknown env restarted: the run does not test the restart's store"
    assert int((env._marker >= 0).sum()) > 0 and int((env._marker < 0).sum()) > 0
    env.check_errors()


@pytest.mark.gpu
def test_a_marked_wavefront_reads_the_pool_not_its_grids():
    spec, B = spec16(max_steps=1024), THROUGHPUT
    g, a = empty_pool()
    other = g.copy()
    other[0, 1, 3] = (6, 2, 0)                                 # a ball two cells in front of the agents at (1, 1)
    true_env, tricked = make_env(spec, B, (g, a)), make_env(spec, B, (g, a))
    over = BatchedMultiGridEnv(spec, B, DEV)                   # the overwritten grid, loaded the regular way
    over.load_state(other[0], a[0], rng=rnglib.synthetic_words(B, 3, 0), step_count=(np.arange(B) % 8).astype(np.int32))
    over.set_layout_pool(g, a)
    assert int((over._marker >= 0).sum()) == 0 and int((tricked._marker == 0).sum()) == B
    for e in (true_env, tricked, over):
        e.step_count.zero_()                                   # (nobody truncates and restarts within the two steps)
    tricked._cells.copy_(over._cells)                          # behind the marker's back
    noop = torch.full((B, 4), 6, dtype=torch.int8, device=DEV)     # `done`: nobody moves, nothing is written
    for e in (true_env, tricked, over):
        e.step(noop, auto_reset=True)
    assert torch.equal(tricked.obs, true_env.obs) and not torch.equal(tricked.obs, over.obs)
    tricked._marker.fill_(-1)
    for e in (tricked, over):
        e.step(noop, auto_reset=True)
    assert torch.equal(tricked.obs, over.obs)


def _ops():
    def read_cells(e):
        return e.cells

    def rollout(e):
        e.rollout(actions(3, e.batch, seed=21), auto_reset=True)

    def persistent(e):
        a = actions(2, e.batch, seed=22)
        with e.persistent(max_steps=2, auto_reset=True) as ps:
            ps.step(a[0]); ps.step(a[1])

    def plain_step(e):
        e.step(actions(1, e.batch, seed=23)[0], auto_reset=False)

    return {"cells": read_cells, "rollout": rollout, "persistent": persistent, "step": plain_step}


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["cells", "rollout", "persistent", "step"])
def test_writers_that_do_not_keep_the_marker_take_the_promise_back(op):
    spec, B = spec16(), 256
    e1, e2 = make_env(spec, B, empty_pool()), make_env(spec, B, empty_pool())
    step2 = untracked_stepper(e2)
    acts = actions(8, B, seed=31)
    for t in range(4):
        e1.step(acts[t], auto_reset=True); step2(acts[t])
    assert int((e1._marker == 0).sum()) == B and e1._mark["armed"]
    _ops()[op](e1)
    assert int((e1._marker >= 0).sum()) == 0, f"{op} left marked envs behind"
    if op != "cells":
        _ops()[op](e2)                                         # (the twin steps untracked: its marker is never looked at)
    for t in range(4, 8):
        e1.step(acts[t], auto_reset=True); step2(acts[t])
        assert_same(e1, e2, f"after {op}, step {t}")
        assert holds(e1)
    assert int((e1._marker == 0).sum()) > 0                    # the restarts armed it again


@pytest.mark.gpu
def test_a_layout_generator_ends_the_tracking():
    e = make_env(spec16(), 128, empty_pool())
    e.step(actions(1, 128)[0], auto_reset=True)
    assert e._mark["armed"]
    e.set_layout_generator("empty_fixed", 1)
    assert int((e._marker >= 0).sum()) == 0 and not e._tracks()
    e.step(actions(1, 128)[0], auto_reset=True)
    assert int((e._marker >= 0).sum()) == 0 and (True, False) in e._bound and not e._bound[(True, False)][2]


@pytest.mark.gpu
def test_state_dict_split_and_graph():
    spec, B = spec16(), 256
    e1, e2 = make_env(spec, B, empty_pool()), make_env(spec, B, empty_pool())
    step2 = untracked_stepper(e2)
    acts = actions(12, B, seed=41)
    # a checkpoint does not carry the marker; loading one compares again
    sd = e1.state_dict()
    assert not any("mark" in k or "layout" in k for k in sd)
    e1._marker.fill_(-1)
    e1.load_state_dict(sd)
    assert int((e1._marker == 0).sum()) == B
    # sub-shards hold slices of the marker and step tracked
    shards = e1.split(2)
    assert [s._marker.data_ptr() for s in shards] == [e1._marker.data_ptr(), e1._marker[128:].data_ptr()]
    assert all(s._mark is e1._mark for s in shards)
    for t in range(4):
        for s, (lo, hi) in zip(shards, ((0, 128), (128, 256))):
            s.step(acts[t, lo:hi].contiguous(), auto_reset=True)
        step2(acts[t])
        assert_same(e1, e2, f"sub-shards, step {t}")
    assert all(s._bound[(True, False)][2] for s in shards)
    # a captured graph of tracked steps equals the eager ones
    graph = e1.capture_steps(acts[4:12], auto_reset=True)
    assert graph._tracked
    graph.replay()
    for t in range(4, 12):
        step2(acts[t])
    assert_same(e1, e2, "graph of 8 tracked steps")
    assert holds(e1) and int((e1._marker == 0).sum()) == B


def test_marker_bookkeeping_on_the_oracle_backend():
    """Arming and disarming without a GPU: the oracle backend steps without the marker, so every step takes the promise back."""
    spec, B = spec16(), 96
    g, a = empty_pool()
    env = make_env(spec, B, (g, a), device="cpu", backend=SelectOracle(spec))
    assert env._tracks() and env._mark["armed"] and int((env._marker == 0).sum()) == B        # one layout: compared at set_layout_pool
    act = torch.from_numpy(util.random_actions(B, 4, 1))
    env.step(act, auto_reset=True)                             # a launcher that does not keep the marker
    assert int((env._marker >= 0).sum()) == 0 and not env._mark["armed"]
    env._marker[:] = 5                                         # not armed: no fill is paid, whatever the tensor holds
    env.step(act, auto_reset=True)
    assert int((env._marker == 5).sum()) == B
    env._marker.fill_(-1)
    env.step_count[:10] = spec.max_steps                       # ten finished envs: reset_done marks exactly them
    env.reset_done()
    assert env._mark["armed"] and torch.equal(env._marker >= 0, env.was_reset.bool()) and int(env.was_reset.sum()) >= 10
    assert env.cells is env._cells and int((env._marker >= 0).sum()) == 0 and not env._mark["armed"]     # handing out the tensor
    mask = torch.zeros(B, dtype=torch.bool)
    mask[3::7] = True
    env.reset(mask=mask)
    assert torch.equal(env._marker == 0, mask)
    shards = env.split(1) if B < 128 else env.split(2)
    assert all(s._mark is env._mark for s in shards) and shards[0]._marker.data_ptr() == env._marker.data_ptr()
    sd = env.state_dict()
    assert "marker" not in sd and "grid_layout" not in sd
    env._marker.fill_(0)
    env._mark["armed"] = True
    env.rollout(torch.from_numpy(np.stack([util.random_actions(B, 4, 2)] * 2)))
    assert int((env._marker >= 0).sum()) == 0
    env.load_state_dict(sd)
    assert env._mark["armed"] and holds(env)
    # a pool of several layouts: nothing is compared, everything starts unknown; a restart cannot name its layout on the host
    g4, a4 = object_pool(4)
    env4 = make_env(spec, B, (g4, a4), device="cpu", backend=SelectOracle(spec))
    assert int((env4._marker >= 0).sum()) == 0 and not env4._mark["armed"]
    env4.reset()
    assert int((env4._marker >= 0).sum()) == 0
