"""Snapshot, restore and fork of chosen envs (include/mgx.h "ENV COPY", BatchedMultiGridEnv.snapshot / restore / fork) without a GPU.

`model_env_copy` is the rule of mgx_env_copy written down sequentially in NumPy.  The host logic of BatchedMultiGridEnv -- which state
set is the source and which the destination, which members they carry, the staging tags and their mode, when the layout markers
survive -- is driven through `CopyOracle`, the episode-accounting oracle launcher plus an `env_copy` that IS the model.
tests/test_env_snapshot_gpu.py holds the kernel to the same model byte for byte.  Also here: the C ABI's refusals (they return
before any HIP call), the exports, the ctypes struct's layout, and the launch geometry of mgx_aux_geom.h walked by a stand-alone
host program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSnapshot, EnvSpec, _lib, layouts
from tests.test_episode_stats import StatsOracle, actions_for, empty_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
MEMBERS = [n for n, _ in _lib.MgxEnvRows._fields_[:-1]]
TRIO = ("cur_return", "cur_length", "over")
NONE, CANDIDATES, SNAPSHOTS = _lib.STAGE_NONE, _lib.STAGE_CANDIDATES, _lib.STAGE_SNAPSHOTS


# ---- the model ---------------------------------------------------------------------------------------------------------------------

def model_env_copy(n, src, src_rows, src_idx, dst, dst_rows, dst_idx, stage_tag, stage_mode, marker_fill, bad):
    """include/mgx.h mgx_env_copy, pair by pair, in place on the dict of arrays `dst` (a missing or None member: the set has no
    such row), `stage_tag` and `bad`."""
    has = lambda rows, m: rows.get(m) is not None
    for i in range(n):
        s = i if src_idx is None else int(src_idx[i])
        d = i if dst_idx is None else int(dst_idx[i])
        if not (0 <= s < src_rows and 0 <= d < dst_rows):
            if bad is not None:
                bad[0] += 1
                bad[1] = min(int(bad[1]), min(i, INT32_MAX))
            continue
        for m in MEMBERS:
            if m != "marker" and m not in TRIO and has(src, m) and has(dst, m):
                dst[m][d] = src[m][s]
        if has(dst, "marker"):
            dst["marker"][d] = src["marker"][s] if has(src, "marker") and not marker_fill else -1
        if has(dst, "cur_length"):
            for m in TRIO:
                dst[m][d] = src[m][s] if has(src, "cur_length") else 0
        if stage_tag is not None and stage_mode == CANDIDATES:
            stage_tag[d, :] = -1
        elif stage_tag is not None and stage_mode == SNAPSHOTS:
            stage_tag[d, 0] = -1
            stage_tag[d, 3] = 0


def test_the_model_on_a_worked_example():
    def rows(n, base, members):
        out = {"cells": np.arange(n * 4, dtype=np.uint8).reshape(n, 2, 2) + base, "agents": np.full((n, 1, 8), base, np.uint8),
               "rng": np.full((n, 4), base, np.int64), "step_count": np.arange(n, dtype=np.int32) + base}
        if "marker" in members:
            out["marker"] = np.arange(n, dtype=np.int32) + base
        if "trio" in members:
            out.update(cur_return=np.full((n, 1), base + 0.5), cur_length=np.full(n, base, np.int32), over=np.ones(n, np.uint8))
        return out
    src, dst = rows(3, 100, ("marker",)), rows(4, 0, ("marker", "trio"))
    tag, bad = np.full((4, 4), 9, np.int32), np.array([0, INT32_MAX], np.int32)
    model_env_copy(4, src, 3, np.array([2, 2, 3, 0]), dst, 4, np.array([0, 3, 1, -1]), tag, SNAPSHOTS, 0, bad)
    assert bad.tolist() == [2, 2]                                          # pairs 2 (source row 3 of 3) and 3 (destination -1)
    assert dst["step_count"].tolist() == [102, 1, 2, 102] and dst["marker"].tolist() == [102, 1, 2, 102]
    assert dst["cells"][3].tolist() == src["cells"][2].tolist() and dst["cells"][1].tolist() == [[4, 5], [6, 7]]
    assert dst["cur_length"].tolist() == [0, 0, 0, 0] and dst["over"].tolist() == [0, 1, 1, 0]      # no source trio: a fresh episode
    assert tag.tolist() == [[-1, 9, 9, 0], [9] * 4, [9] * 4, [-1, 9, 9, 0]]
    model_env_copy(1, src, 3, None, dst, 4, np.array([2]), tag, CANDIDATES, 1, None)
    assert dst["marker"].tolist() == [102, 1, -1, 102] and tag[2].tolist() == [-1] * 4 and dst["step_count"][2] == 100


# ---- the host logic over the model -------------------------------------------------------------------------------------------------

class CopyOracle(StatsOracle):
    """StatsOracle + env_copy, which is the model; `copies` records (n, source members, destination members, mode, marker_fill)."""

    def __init__(self, spec):
        super().__init__(spec)
        self.copies = []

    def env_copy(self, n, src, src_rows, src_idx, dst, dst_rows, dst_idx, stage_tag, stage_mode, marker_fill, bad):
        self.copies.append((n, sorted(src), sorted(dst), stage_mode, bool(marker_fill)))
        assert (stage_tag is None) == (stage_mode == NONE)
        as_np = lambda t: None if t is None else t.numpy()
        model_env_copy(n, self._np(src), src_rows, as_np(src_idx), self._np(dst), dst_rows, as_np(dst_idx), as_np(stage_tag), stage_mode,
                       marker_fill, as_np(bad))


SPEC = EnvSpec(5, 5, 2, 3, max_steps=6)
FORMS = ("plain", "pool", "gen", "gen_candidates", "gen_between")
STATE = ("_cells", "agents", "rng", "step_count", "aux")
OUTPUTS = ("obs", "dir", "reward", "terminated", "truncated")


def make_env(form, B=7, spec=SPEC, dev="cpu", backend=None, first_env=0, pool_size=2):
    """form: 'plain' (no restart source: the state is loaded), 'pool', 'gen' (device generator, unstaged), 'gen_candidates' /
    'gen_between' (the same generator with staging slots)"""
    kw = {"backend": backend} if backend is not None else {}
    env = BatchedMultiGridEnv(spec, B, dev, first_env=first_env, **kw)
    pg, pa = empty_pool(spec)
    if form == "plain":
        env.load_state(pg[0], pa[0])
        env.seed(3)
    elif form == "pool":
        env.set_layout_pool(pg[:pool_size], pa[:pool_size])
        env.reset(seed=3)
    else:
        staged = {"gen": False, "gen_candidates": "candidates", "gen_between": "between"}[form]
        env.set_layout_generator("empty_random", layout_seed=5, staged=staged, lead=4)
        env.reset(seed=3)
        stage = env._gen.get("stage")
        assert (stage is None) == (form == "gen")
        if stage is not None:
            assert bool(stage.get("candidates")) == (form == "gen_candidates") and stage["external"] == 2
    return env


def state_of(env):
    out = {k: getattr(env, k).cpu().numpy().copy() for k in STATE}
    if getattr(env, "episode", None) is not None:
        out["episode"] = env.episode.cpu().numpy().copy()
    if getattr(env, "_gen", None) is not None:
        out["gen_state"] = env._gen["gen_state"].cpu().numpy().copy()
    return out


def run(env, acts, auto_reset):
    """the outputs of every step (and was_reset with auto-reset), then the final state"""
    steps = []
    for t in range(acts.shape[0]):
        env.step(acts[t], auto_reset=auto_reset)
        steps.append({k: getattr(env, k).cpu().numpy().copy() for k in OUTPUTS + (("was_reset",) if auto_reset else ())})
    return steps, state_of(env)


def assert_same_run(a, b, ctx=""):
    (sa, fa), (sb, fb) = a, b
    for t, (x, y) in enumerate(zip(sa, sb)):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), f"{ctx}: step {t}: {k}"
    assert set(fa) == set(fb)
    for k in fa:
        assert fa[k].tobytes() == fb[k].tobytes(), f"{ctx}: final {k}"


def poison_tags(env):
    """(the oracle launcher never stages: the tags are filled by hand, recognisably)"""
    tag = env._gen["stage"]["tag"]
    tag.copy_(torch.arange(tag.numel(), dtype=torch.int32).reshape(tag.shape) + 100)
    return tag.numpy().copy()


def tags_after(before, written, candidates):
    want = before.copy()
    if candidates:
        want[written] = -1
    else:
        want[written, 0] = -1
        want[written, 3] = 0
    return want


@pytest.mark.parametrize("B", [7, 130])
@pytest.mark.parametrize("form", FORMS)
def test_a_restored_batch_repeats_its_run(form, B):
    be = CopyOracle(SPEC)
    env = make_env(form, B=B, backend=be)
    A, T, ar = SPEC.num_agents, 2 * SPEC.max_steps + 3, form != "plain"
    env.step(actions_for(B, A, 1, 9)[0], auto_reset=ar)                    # (not at a fresh start: mid-episode)
    snap = env.snapshot()
    assert isinstance(snap, EnvSnapshot) and snap.rows == B and snap.spec == SPEC
    members = {"cells", "agents", "rng", "step_count", "aux", "marker"} | ({"episode"} if ar else set()) \
        | ({"gen_state"} if form.startswith("gen") else set())
    assert set(snap.tensors) == members
    assert snap.nbytes == sum(t.numel() * t.element_size() for t in snap.tensors.values()) > B * (25 * 2 + A * 8 + 32 + 4 + 16)
    acts = actions_for(B, A, T, 1)
    first = run(env, acts, ar)
    if ar:
        assert (env.episode.numpy() >= 3).all(), "every env goes through two episode ends"
    staged = form in ("gen_candidates", "gen_between")
    before = poison_tags(env) if staged else None
    assert env.restore(snap) is None
    assert be.copies[-1][3] == {"gen_candidates": CANDIDATES, "gen_between": SNAPSHOTS}.get(form, NONE)
    if staged:
        assert env._gen["stage"]["tag"].numpy().tolist() == tags_after(before, np.arange(B), form == "gen_candidates").tolist()
    for k, t in snap.tensors.items():                                       # the snapshot is a value: restoring does not change it
        assert t.data_ptr() != env._state_rows()[k].data_ptr()
    assert_same_run(run(env, acts, ar), first, form)
    env.check_errors()
    # out=: the same tensors are written again
    ptrs = {k: t.data_ptr() for k, t in snap.tensors.items()}
    assert env.snapshot(out=snap) is snap and {k: t.data_ptr() for k, t in snap.tensors.items()} == ptrs
    assert snap.tensors["step_count"].tolist() == env.step_count.tolist()


@pytest.mark.parametrize("form", ["pool", "gen", "gen_candidates"])
def test_forks_of_one_source_run_alike(form):
    B, A, T = 130, SPEC.num_agents, 2 * SPEC.max_steps + 3
    env = make_env(form, B=B, backend=CopyOracle(SPEC))
    for a in actions_for(B, A, 3, 4):                                      # (the sources differ from each other by now)
        env.step(a, auto_reset=True)
    src = torch.tensor([5, 64, 129])
    r = np.random.default_rng(0)
    dst = torch.from_numpy(np.sort(r.permutation(B)[:100]))
    rows = torch.from_numpy(r.integers(0, 3, size=100))
    snap = env.snapshot(src)
    assert snap.rows == 3
    untouched = np.setdiff1d(np.arange(B), dst.numpy())
    before = state_of(env)
    env.restore(snap, dst, rows)
    after = state_of(env)
    for k in before:
        assert after[k][untouched].tobytes() == before[k][untouched].tobytes(), k
        assert after[k][dst.numpy()].tobytes() == snap.tensors[k.lstrip("_")].numpy()[rows.numpy()].tobytes(), k
    acts = actions_for(B, A, T, 2)
    for j in range(3):                                                     # every fork of a source gets its source's actions
        acts[:, dst[rows == j]] = acts[:, int(dst[rows == j][0])].unsqueeze(1)
    steps, _ = run(env, acts, True)
    for j in range(3):
        group = dst.numpy()[rows.numpy() == j]
        assert len(group) > 20
        upto = T
        if form == "pool":                                                  # ... up to the first restart: the slot's own layout from there
            restarts = [t for t in range(T) if steps[t]["was_reset"][group].any()]
            assert restarts and all(steps[restarts[0]]["was_reset"][group])
            upto = restarts[0]
        for t in range(upto):
            for k in OUTPUTS:
                x = steps[t][k][group]
                assert (x == x[:1]).all(), (form, j, t, k)
    if form == "pool":
        assert any(len({steps[-1]["obs"][b].tobytes() for b in dst.numpy()[rows.numpy() == j]}) > 1 for j in range(3)), \
            "after a restart the slots' own layouts part the forks"
    # fork() = restore(snapshot(src), dst)
    twin = make_env(form, B=B, backend=CopyOracle(SPEC))
    ref = make_env(form, B=B, backend=CopyOracle(SPEC))
    s2, d2 = torch.tensor([1, 1, 2]), torch.tensor([2, 7, 1])              # (env 2 is a source and a destination: it hands on its OLD state)
    for a in actions_for(B, A, 3, 4):
        twin.step(a, auto_reset=True); ref.step(a, auto_reset=True)
    twin.fork(s2, d2)
    ref.restore(ref.snapshot(s2), d2)
    for k, v in state_of(ref).items():
        assert state_of(twin)[k].tobytes() == v.tobytes(), k
    assert twin.agents[1].tolist() == ref.agents[1].tolist() != twin.agents[2].tolist() == twin.agents[7].tolist()


@pytest.mark.parametrize("form", ["gen_candidates", "gen_between"])
def test_a_restore_drops_the_staging_slots_of_the_envs_it_writes(form):
    B, A = 130, SPEC.num_agents
    env, plain = make_env(form, B=B, backend=CopyOracle(SPEC)), make_env("gen", B=B, backend=CopyOracle(SPEC))
    for a in actions_for(B, A, 2, 4):
        env.step(a, auto_reset=True); plain.step(a, auto_reset=True)
    src, dst = torch.tensor([3, 70]), torch.tensor([0, 64, 65, 129])
    rows = torch.tensor([0, 1, 1, 0])
    before = poison_tags(env)
    env.restore(env.snapshot(src), dst, rows)
    plain.restore(plain.snapshot(src), dst, rows)
    assert env._gen["stage"]["tag"].numpy().tolist() == tags_after(before, dst.numpy(), form == "gen_candidates").tolist()
    acts = actions_for(B, A, SPEC.max_steps + 2, 6)
    assert_same_run(run(env, acts, True), run(plain, acts, True), form)
    assert (env.episode.numpy() >= 2).all()


def test_the_layout_marker_survives_only_where_it_means_something():
    spec, B = SPEC, 7
    be = CopyOracle(spec)
    env = make_env("pool", B=B, backend=be, pool_size=1)                   # one layout: the restart marks every env 0, armed
    assert env._tracks() and env._mark["armed"] and env._marker.tolist() == [0] * B
    snap = env.snapshot()
    assert snap.tensors["marker"].tolist() == [0] * B and snap.layout_version == env._layout_version
    env.step(actions_for(B, 2, 1, 1)[0])                                    # (a step that does not keep the marker)
    assert not env._mark["armed"] and env._marker.tolist() == [-1] * B
    ids = torch.tensor([1, 4])
    env.restore(snap, ids, ids)                                             # same env, same version: kept, and armed again
    assert env._marker.tolist() == [-1, 0, -1, -1, 0, -1, -1] and env._mark["armed"] and be.copies[-1][4] is False
    # the pool refilled (in place: _layout_version stays, the layouts do not): the indices mean nothing any more
    pg, pa = empty_pool(spec)
    env.set_layout_pool(pg[1:2], pa[1:2])
    assert env._layout_version == snap.layout_version and env._marker.tolist() == [0] * B      # (the two layouts' cells are equal)
    env.restore(snap, ids, ids)
    assert env._marker.tolist() == [0, -1, 0, 0, -1, 0, 0] and be.copies[-1][4] is True
    assert (env._cells[ids] == snap.tensors["cells"][ids]).all()
    # another env object of equal spec and restart source
    other = make_env("pool", B=B, backend=CopyOracle(spec), pool_size=1)
    other.step(actions_for(B, 2, 1, 1)[0])
    assert not other._mark["armed"]
    other.restore(make_env("pool", B=B, backend=CopyOracle(spec), pool_size=1).snapshot())
    assert other._marker.tolist() == [-1] * B and not other._mark["armed"] and other.backend.copies[-1][4] is True
    # a snapshot taken while nothing was marked does not arm
    env2 = make_env("pool", B=B, backend=CopyOracle(spec), pool_size=1)
    env2.step(actions_for(B, 2, 1, 1)[0])
    s2 = env2.snapshot()
    env2.restore(s2)
    assert not env2._mark["armed"] and env2._marker.tolist() == [-1] * B


def test_the_running_episode_travels_and_the_totals_stay():
    B, A = 7, SPEC.num_agents
    env = make_env("pool", B=B, backend=CopyOracle(SPEC))
    untracked = env.snapshot()
    stats = env.track_episodes()
    acts = actions_for(B, A, 12, 8)
    for t in range(3):
        env.step(acts[t], auto_reset=True)
    stats.cur_return.add_(torch.arange(B * A, dtype=torch.float64).reshape(B, A) + 0.5)      # (Empty pays at the end only: recognisable)
    snap = env.snapshot()
    assert set(TRIO) <= set(snap.tensors) and not set(TRIO) & set(untracked.tensors)
    at_snap = {n: t.numpy().copy() for n, t in stats.tensors.items()}
    assert at_snap["cur_length"].any() and at_snap["cur_return"].any()
    for t in range(3, 12):
        env.step(acts[t], auto_reset=True)
    later = {n: t.numpy().copy() for n, t in stats.tensors.items()}
    assert later["counts"][:, 0].all()
    env.restore(snap)
    for n, t in stats.tensors.items():
        assert t.numpy().tobytes() == (at_snap if n in TRIO else later)[n].tobytes(), n
    # a snapshot without the trio: a fresh episode in every env it writes, and nothing is counted
    env.step(acts[0], auto_reset=True)
    running = {n: t.numpy().copy() for n, t in stats.tensors.items()}
    ids = torch.from_numpy(np.flatnonzero(running["cur_length"] > 0)[:3])
    assert len(ids) >= 2
    env.restore(untracked, ids, ids)
    got = {n: t.numpy().copy() for n, t in stats.tensors.items()}
    keep = np.setdiff1d(np.arange(B), ids.numpy())
    for n in stats.tensors:
        if n in TRIO:
            assert not got[n][ids.numpy()].any() and got[n][keep].tobytes() == running[n][keep].tobytes(), n
        else:
            assert got[n].tobytes() == running[n].tobytes(), n
    # ... and a snapshot WITH it restores into an env that does not track: the trio is left alone
    env.track_episodes(None)
    env.restore(snap)
    assert env.step_count.tolist() == snap.tensors["step_count"].tolist()


def test_refusals_and_the_bad_pair_counter():
    B = 130
    env = make_env("pool", B=B, backend=CopyOracle(SPEC))
    snap = env.snapshot()
    ids = torch.arange(4)
    # a persistent session is open
    env._session = object()
    for call in (lambda: env.snapshot(), lambda: env.restore(snap), lambda: env.fork(ids, ids + 4)):
        with pytest.raises(RuntimeError, match="persistent session"):
            call()
    env._session = None
    # no state is loaded
    empty = BatchedMultiGridEnv(SPEC, B, "cpu", backend=CopyOracle(SPEC))
    for call in (lambda: empty.snapshot(), lambda: empty.restore(snap), lambda: empty.fork(ids, ids + 4)):
        with pytest.raises(RuntimeError, match="no state loaded"):
            call()
    # a child of split()
    child = env.split(2)[0]
    for call in (lambda: child.snapshot(), lambda: child.restore(snap), lambda: child.fork(ids, ids + 4)):
        with pytest.raises(RuntimeError, match="sub-shard of split"):
            call()
    # another spec; another kind of restart source
    with pytest.raises(ValueError, match="different EnvSpec"):
        spec7 = EnvSpec(5, 5, 2, 3, max_steps=7)
        make_env("pool", B=B, spec=spec7, backend=CopyOracle(spec7)).restore(snap)
    for form in ("plain", "gen"):
        with pytest.raises(ValueError, match="restart source"):
            make_env(form, B=B, backend=CopyOracle(SPEC)).restore(snap)
    gen = make_env("gen", B=B, backend=CopyOracle(SPEC))
    other_kind = BatchedMultiGridEnv(SPEC, B, "cpu", backend=CopyOracle(SPEC))
    other_kind.set_layout_generator("empty_fixed", layout_seed=5, staged=False)
    other_kind.reset(seed=3)
    with pytest.raises(ValueError, match="restart source"):
        other_kind.restore(gen.snapshot())
    with pytest.raises(TypeError, match="EnvSnapshot"):
        env.restore({"cells": env._cells})
    # the index tensors: dtype, shape, contiguity, device
    bad_ids = (torch.arange(4, dtype=torch.int32), torch.arange(4).reshape(2, 2), torch.arange(8)[::2], [0, 1, 2, 3],
               torch.zeros(4, dtype=torch.int64, device="meta"))
    for t in bad_ids:
        with pytest.raises(ValueError, match="env_ids must be a contiguous int64 tensor"):
            env.snapshot(t)
        with pytest.raises(ValueError, match="env_ids must be a contiguous int64 tensor"):
            env.restore(snap, t)
        with pytest.raises(ValueError, match="rows must be a contiguous int64 tensor"):
            env.restore(snap, ids, t)
        with pytest.raises(ValueError, match="src_ids must be a contiguous int64 tensor"):
            env.fork(t, ids)
        with pytest.raises(ValueError, match="dst_ids must be a contiguous int64 tensor"):
            env.fork(ids, t)
    with pytest.raises(ValueError, match="rows has 3 entries for 4"):
        env.restore(snap, ids, torch.arange(3))
    with pytest.raises(ValueError, match="rows has 4 entries for 130"):
        env.restore(snap, None, ids)
    with pytest.raises(ValueError, match="3 source.s. for 4"):
        env.fork(torch.arange(3), ids)
    small = env.snapshot(ids)
    with pytest.raises(ValueError, match="holds 4 row"):
        env.restore(small)
    # out= of another shape / member set
    with pytest.raises(ValueError, match="out= has another shape"):
        env.snapshot(out=small)
    with pytest.raises(ValueError, match="out= has another shape"):
        env.snapshot(torch.arange(5), out=small)
    with pytest.raises(ValueError, match="out= has another shape"):
        gen.snapshot(ids, out=small)
    env.track_episodes()
    with pytest.raises(ValueError, match="out= has another shape"):
        env.snapshot(ids, out=small)
    env.track_episodes(None)
    assert env.snapshot(ids, out=small) is small
    # check=True: a synchronising look at the ids
    with pytest.raises(ValueError, match="more than once"):
        env.restore(small, torch.tensor([1, 2, 1, 0]), check=True)
    with pytest.raises(ValueError, match=r"env_ids must lie in \[0, 130\)"):
        env.restore(small, torch.tensor([1, 2, 130, 0]), check=True)
    with pytest.raises(ValueError, match=r"rows must lie in \[0, 4\)"):
        env.restore(small, ids, torch.tensor([0, 1, 4, 2]), check=True)
    with pytest.raises(ValueError, match=r"src_ids must lie in \[0, 130\)"):
        env.fork(torch.tensor([0, -1]), torch.tensor([5, 6]), check=True)
    with pytest.raises(ValueError, match="more than once"):
        env.fork(torch.tensor([0, 1]), torch.tensor([5, 5]), check=True)
    env.restore(small, torch.tensor([9, 8, 7, 6]), torch.tensor([0, 0, 3, 3]), check=True)
    env.check_errors()
    # without it the kernel skips the pair and counts it: check_errors() tells
    before = state_of(env)
    env.restore(small, torch.tensor([1, 2, 130, 0]), torch.tensor([0, 1, 2, 7]))
    after = state_of(env)
    assert after["agents"][3:].tobytes() == before["agents"][3:].tobytes() and after["agents"][0].tobytes() == before["agents"][0].tobytes()
    env.snapshot(torch.tensor([-5, 0, 1, 2]), out=small)
    with pytest.raises(ValueError, match=r"3 pair\(s\) named an env id or a snapshot row out of range.*first at pair 0"):
        env.check_errors()
    env.check_errors()                                                      # (reported once)
    env.err[0] = 1                                                          # the unknown-action clause is what it was, and comes first
    env.err[1] = 2
    env.restore(small, torch.tensor([1, 2, 130, 0]))
    with pytest.raises(ValueError, match="Unknown action in 1 env"):
        env.check_errors()
    with pytest.raises(ValueError, match="1 pair.s. named"):
        env.check_errors()


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------------

def test_c_abi_argument_validation():
    """what mgx_env_copy checks of its own; the checks of every row query, on either of its two sets: tests/test_row_query_abi.py"""
    from tests.test_row_query_abi import INV, P as p, full, ref
    L = _lib.lib()
    assert L.mgx_abi_version() == 11
    sc = EnvSpec(5, 5, 2, 3, max_steps=4).to_c()

    def E(sc_, n, src, dst, src_idx=p, dst_idx=p, tag=p, mode=1, fill=0, bad=p):
        return L.mgx_env_copy(ref(sc_), n, ref(src), src_idx, ref(dst), dst_idx, tag, mode, fill, bad, None)
    a, b = full(), full()
    for mode in (-1, 3):
        assert E(sc, 4, a, b, mode=mode) == INV and E(sc, 0, a, b, mode=mode) == INV
    # the running trio: all three or none
    for k in range(1, 7):
        part = {m: None for j, m in enumerate(TRIO) if not (k >> j) & 1}
        assert E(sc, 4, full(**part), b) == INV and E(sc, 4, a, full(**part)) == INV, part
    # alignment: 8 bytes for the destination's indices, 16 for the staging tags
    assert E(sc, 4, a, b, dst_idx=p + 4) == INV
    assert E(sc, 4, a, b, tag=p + 8) == INV


def test_the_export_is_the_headers_declaration():
    from tests.test_capi import declared_functions
    names = declared_functions()
    assert "mgx_env_copy" in names and "mgx_env_copy" in _lib.EXPORTS and set(names) == set(_lib.EXPORTS)
    assert _lib.lib().mgx_env_copy is not None and _lib.lib().mgx_abi_version() == _lib.ABI_VERSION == 11


def test_the_ctypes_struct_matches_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    cls = _lib.MgxEnvRows
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mgx.h"', 'int main(void) {',
             '  printf("MgxEnvRows %zu", sizeof(MgxEnvRows));']
    lines += [f'  printf(" %zu", offsetof(MgxEnvRows, {f}));' for f, _ in cls._fields_]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert out == ["MgxEnvRows"] + [str(v) for v in [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]]
    assert [f for f, _ in cls._fields_] == MEMBERS + ["rows"] and EnvSnapshot.MEMBERS == tuple(MEMBERS)


# ---- the launch geometry, by a stand-alone host program under the sanitizers -------------------------------------------------------

GEOMETRY_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "mgx_aux_geom.h"
using namespace mgx;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s: tile %d n %lld\n", #c, tile, (long long)n); return 1; } } while (0)
int main() {
    long long walked = 0;
    std::vector<int> seen(5000);
    for (int tile = 1; tile <= 8192; ++tile) {
        long long n = 0;
        // the copy unit: divides the tile and both bases, and is the widest that does -- by size, and by address
        for (int ks = 0; ks < 4; ++ks)
            for (int kd = 0; kd < 4; ++kd) {
                const uintptr_t s = 4096 + (uintptr_t)ks * tile, d = 8192 + (uintptr_t)kd * tile;
                const ResetUnit u = env_copy_unit(tile, s, d);
                CHECK(u.unit == 16 || u.unit == 8 || u.unit == 4 || u.unit == 2 || u.unit == 1);
                CHECK(tile % u.unit == 0 && s % u.unit == 0 && d % u.unit == 0 && u.units * u.unit == tile && u.units >= 1);
                const int w = 2 * u.unit;
                CHECK(u.unit == 16 || tile % w || s % w || d % w);
                // every row of either set is aligned to the unit
                for (int r = 0; r < 5; ++r) CHECK((s + (uintptr_t)r * tile) % u.unit == 0 && (d + (uintptr_t)r * tile) % u.unit == 0);
            }
        const int bound = tile > kEnvCopyWaveBytes ? tile : kEnvCopyWaveBytes;
        for (n = 1; n <= 5000; ++n) {
            const EnvCopyGeom g = env_copy_geom(tile, n);
            CHECK(g.run >= 1 && g.run <= 64);
            CHECK((long long)g.run * tile <= bound);                                  // a wavefront's tile bytes
            CHECK(g.nwaves >= 1 && (g.nwaves - 1) * g.run < n && g.nwaves * g.run >= n);   // the last wavefront has a pair, none is left over
            CHECK(g.blocks * kEnvCopyWpb >= g.nwaves && (g.blocks - 1) * kEnvCopyWpb < g.nwaves);
            CHECK(g.run == 1 || g.nwaves >= kEnvCopyFillWaves || g.run == (kEnvCopyWaveBytes / tile > 64 ? 64 : kEnvCopyWaveBytes / tile));
            if (tile >= kEnvCopyWaveBytes) CHECK(g.run == 1 && g.nwaves == n);         // (64 envs of 64x64: 64 wavefronts)
            if ((tile % 97 == 1 && n % 10 == 3) || n % 1250 == 0 || n <= 2) {          // the pairs, one by one: [0, n) exactly once
                for (long long i = 0; i < n; ++i) seen[i] = 0;
                for (long long w = 0; w < g.blocks * kEnvCopyWpb; ++w) {
                    const long long p0 = w * g.run;
                    if (p0 >= n) { CHECK(w >= g.nwaves); continue; }
                    CHECK(w < g.nwaves);
                    int pairs = 0;
                    for (int lane = 0; lane < g.run; ++lane)                           // (the kernel: lane < run && p0 + lane < n)
                        if (p0 + lane < n) { seen[p0 + lane]++; pairs++; }
                    CHECK(pairs >= 1);
                }
                for (long long i = 0; i < n; ++i) CHECK(seen[i] == 1);
                walked++;
            }
        }
    }
    printf("ok %lld\n", walked);
    return 0;
}
"""


def test_the_launch_geometry_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no C++ compiler"
    src, exe = tmp_path / "geometry.cpp", tmp_path / "geometry"
    src.write_text(GEOMETRY_MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-I", os.path.join(ROOT, "multigrid_amd", "csrc"), str(src), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-2000:] + p.stderr[-2000:]
    assert int(p.stdout.split()[1]) > 80000
