"""Episode accounting (include/mgx.h "EPISODE ACCOUNTING", BatchedMultiGridEnv.track_episodes) without a GPU.

`model_stats` / `model_restart` are the rule written down sequentially in NumPy: one np.float64 add per accumulation, in the stated
order.  The host logic of BatchedMultiGridEnv -- which accounting call follows which launch, with which restart mode, over which
tensors -- is driven through `StatsOracle`, an oracle launcher whose two new backend calls ARE the model; what it must produce is
computed independently, by feeding the recorded outputs of every step to a fresh model.  tests/test_episode_stats_gpu.py holds the
kernels to the same model bit for bit.  Also here: the C ABI's refusals (they return before any HIP call) and the exports."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib, layouts
from multigrid_amd.batched import EpisodeStats
from tests.test_reset_select import SelectOracle

NONE, BEFORE, AFTER = _lib.RESTART_NONE, _lib.RESTART_BEFORE, _lib.RESTART_AFTER
NAMES = [n for n, _ in _lib.MgxEpisodeStats._fields_]
TRACE = [n for n, _ in _lib.MgxEpisodeTrace._fields_]


# ---- the model ---------------------------------------------------------------------------------------------------------------------

def new_state(B, A):
    return {"cur_return": np.zeros((B, A), np.float64), "cur_length": np.zeros(B, np.int32), "over": np.zeros(B, np.uint8),
            "last_return": np.zeros((B, A), np.float64), "last_length": np.zeros(B, np.int32),
            "sum_return": np.zeros((B, A), np.float64), "sum_length": np.zeros(B, np.int64), "counts": np.zeros((B, 4), np.int32)}


def new_trace(T, B, A, fill=0x5a):
    """(poisoned: the kernel must write every (t, b))"""
    tr = {"closed": np.empty((T, B), np.uint8), "episode_return": np.empty((T, B, A), np.float64),
          "episode_length": np.empty((T, B), np.int32)}
    for v in tr.values():
        v.view(np.uint8).fill(fill)
    return tr


def _restart_clause(st, b, seen):
    if not st["over"][b] and st["cur_length"][b] > 0:
        st["counts"][b, 3] += 1
        st["cur_return"][b] = 0.0
        st["cur_length"][b] = 0
        seen["abort"] = seen.get("abort", 0) + 1
    elif not st["over"][b]:
        seen["restart_at_0"] = seen.get("restart_at_0", 0) + 1
    st["over"][b] = 0


def model_stats(st, reward, terminated, truncated, was_reset, restart, trace=None, seen=None):
    """The update for the outputs of T steps (arrays with or without the leading [T] axis), in place on the dict of arrays `st`."""
    seen = {} if seen is None else seen
    B, A = st["cur_return"].shape
    reward, terminated, truncated = reward.reshape(-1, B, A), terminated.reshape(-1, B, A), truncated.reshape(-1, B)
    if restart != NONE:
        was_reset = was_reset.reshape(-1, B)
    for t in range(reward.shape[0]):
        for b in range(B):
            if restart == BEFORE and was_reset[t, b]:
                _restart_clause(st, b, seen)
            closed, ret, length = False, np.zeros(A, np.float64), 0
            if not st["over"][b]:
                for a in range(A):
                    st["cur_return"][b, a] = np.float64(st["cur_return"][b, a]) + np.float64(reward[t, b, a])
                st["cur_length"][b] += 1
                all_term = bool((terminated[t, b] != 0).all())
                if truncated[t, b] != 0 or all_term:
                    closed, ret, length = True, st["cur_return"][b].copy(), int(st["cur_length"][b])
                    st["last_return"][b] = ret
                    st["last_length"][b] = length
                    for a in range(A):
                        st["sum_return"][b, a] = np.float64(st["sum_return"][b, a]) + ret[a]
                    st["sum_length"][b] += length
                    st["counts"][b, 0] += 1
                    st["counts"][b, 1] += int(all_term)
                    st["counts"][b, 2] += int((ret > 0).any())
                    st["cur_return"][b] = 0.0
                    st["cur_length"][b] = 0
                    st["over"][b] = 1
                    seen["trunc" if truncated[t, b] != 0 and not all_term else ("term" if truncated[t, b] == 0 else "both")] = 1
                    seen["rewarded"] = seen.get("rewarded", 0) + int((ret > 0).any())
                elif (terminated[t, b] != 0).any():
                    seen["partial_term"] = 1
            else:
                seen["skipped"] = seen.get("skipped", 0) + 1
            if trace is not None:
                if trace.get("closed") is not None:
                    trace["closed"][t, b] = closed
                if trace.get("episode_return") is not None:
                    trace["episode_return"][t, b] = ret
                if trace.get("episode_length") is not None:
                    trace["episode_length"][t, b] = length
            if restart == AFTER and was_reset[t, b]:
                _restart_clause(st, b, seen)
    return seen


def model_restart(st, select, seen=None):
    seen = {} if seen is None else seen
    for b in range(st["over"].shape[0]):
        if select is None or select[b]:
            _restart_clause(st, b, seen)
    return seen


def test_the_model_on_a_worked_example():
    st = new_state(2, 2)
    rew = np.array([[[0.5, 0.0], [1.0, 1.0]], [[0.25, 0.0], [9.0, 9.0]], [[1.0, 1.0], [2.0, 0.0]]])
    term = np.array([[[1, 0], [1, 1]], [[1, 1], [1, 1]], [[0, 0], [0, 0]]], np.uint8)
    trunc = np.array([[0, 0], [0, 0], [0, 1]], np.uint8)
    wr = np.array([[0, 0], [0, 0], [1, 1]], np.uint8)
    tr = new_trace(3, 2, 2)
    model_stats(st, rew, term, trunc, wr, BEFORE, tr)
    # env 0: closes at t = 1 by termination (0.75, 0) length 2; restarted before t = 2, runs (1, 1) length 1
    # env 1: closes at t = 0 (1, 1) length 1; t = 1 is a step past the end; restarted before t = 2, truncated there: (2, 0) length 1
    assert st["counts"].tolist() == [[1, 1, 1, 0], [2, 1, 2, 0]]
    assert st["last_return"].tolist() == [[0.75, 0.0], [2.0, 0.0]] and st["sum_return"].tolist() == [[0.75, 0.0], [3.0, 1.0]]
    assert st["cur_return"].tolist() == [[1.0, 1.0], [0.0, 0.0]] and st["cur_length"].tolist() == [1, 0]
    assert st["over"].tolist() == [0, 1] and st["sum_length"].tolist() == [2, 2]
    assert tr["closed"].tolist() == [[0, 1], [1, 0], [0, 1]] and tr["episode_length"].tolist() == [[0, 1], [2, 0], [0, 1]]
    assert tr["episode_return"][1, 0].tolist() == [0.75, 0.0] and not tr["episode_return"][1, 1].any()
    model_restart(st, np.array([1, 0], np.uint8))
    assert st["counts"][:, 3].tolist() == [1, 0] and not st["cur_return"].any() and st["over"].tolist() == [0, 1]


# ---- the host logic over the model -------------------------------------------------------------------------------------------------

class StatsOracle(SelectOracle):
    """The oracle launcher + the two accounting calls, which are the model; `calls` records (what, restart mode, T)."""

    def __init__(self, spec):
        super().__init__(spec)
        self.calls = []

    @staticmethod
    def _np(d):
        return {k: v.numpy() for k, v in d.items() if v is not None}

    def episode_stats(self, B, T, reward, terminated, truncated, was_reset, restart, stats, trace=None):
        self.calls.append(("stats", restart, T))
        assert (was_reset is None) == (restart == NONE)
        model_stats(self._np(stats), reward.numpy(), terminated.numpy(), truncated.numpy(),
                    None if was_reset is None else was_reset.numpy(), restart, None if trace is None else self._np(trace))

    def episode_restart(self, B, select, stats):
        self.calls.append(("restart", None if select is None else int(select.sum()), 0))
        model_restart(self._np(stats), None if select is None else select.numpy())

    def rollout(self, B, T, grid, agents, rng, step_count, actions, target, err, obs, dirs, reward, terminated, truncated,
                auto_reset=None, generate=None):
        for t in range(T):
            kw = {}
            if auto_reset is not None:
                kw["auto_reset"] = auto_reset[:3] + (auto_reset[3][t],)
            self.step(B, grid, agents, rng, step_count, actions[t], target, err, obs[t], dirs[t], reward[t], terminated[t],
                      truncated[t], **kw)
            if generate is not None:
                gen, episode, was_reset = generate
                self.reset_generate(B, gen, grid, agents, rng, step_count, target, episode, was_reset[t])


SPEC = EnvSpec(5, 5, 2, 3, max_steps=4)
FORWARD = 2


def empty_pool(spec):
    """Two starts of an Empty grid: the reference's (agents at (1, 1), facing right), and one cell before the goal, facing it --
    `forward` ends that episode by termination, with a reward"""
    g0, a0 = layouts.empty_layout(spec.width, spec.num_agents)
    g1, a1 = layouts.empty_layout(spec.width, spec.num_agents, agent_start_pos=(spec.width - 3, spec.height - 2), agent_start_dir=0)
    return np.stack([g0, g1]), np.stack([a0, a1])


def actions_for(B, A, T, seed):
    """random actions; every third env only walks forward"""
    a = np.random.default_rng(seed).integers(0, 7, size=(T, B, A)).astype(np.int8)
    a[:, ::3] = FORWARD
    return torch.from_numpy(a)


def make_env(form, B=7, spec=SPEC, dev="cpu", backend=None, first_env=0):
    """form: 'pool' (layout pool), 'gen' (device generator), 'plain' (pool set, but restarts are the caller's)"""
    kw = {"backend": backend} if backend is not None else {}
    env = BatchedMultiGridEnv(spec, B, dev, first_env=first_env, **kw)
    if form == "gen":
        env.set_layout_generator("empty_random", layout_seed=5, staged=False)
        env.reset(seed=3)
    else:
        pg, pa = empty_pool(spec)
        env.set_layout_pool(pg, pa)
        env.reset(seed=3)
    return env


def snapshot(stats):
    return {n: t.cpu().numpy().copy() for n, t in stats.tensors.items()}


def assert_same(got, want, ctx=""):
    for n in NAMES:
        assert got[n].tobytes() == want[n].tobytes(), f"{ctx}: {n}\n{got[n]}\n{want[n]}"


def record(env):
    return [getattr(env, k).cpu().numpy().copy() for k in ("reward", "terminated", "truncated", "was_reset")]


@pytest.mark.parametrize("form", ["pool", "gen"])
def test_step_with_auto_reset_follows_the_rule(form):
    be = StatsOracle(SPEC)
    env = make_env(form, backend=be)
    stats = env.track_episodes()
    assert isinstance(stats, EpisodeStats) and env.episode_stats is stats
    B, A, T = env.batch, SPEC.num_agents, 4 * SPEC.max_steps + 3
    acts = actions_for(B, A, T, 1)
    want, seen = new_state(B, A), {}
    e0 = env.episode.clone()
    for t in range(T):
        env.step(acts[t], auto_reset=True)
        r, te, tr, wr = record(env)
        model_stats(want, r, te, tr, wr, BEFORE if form == "pool" else AFTER, seen=seen)
    assert_same(snapshot(stats), want, form)
    assert seen.get("trunc") and not seen.get("abort"), seen
    assert not stats.counts[:, 3].any()
    if form == "gen":
        assert torch.equal(stats.counts[:, 0], env.episode - e0)
        assert all(c[0] == "stats" and c[1] == NONE for c in be.calls if c[0] == "stats"), "the oracle path: NONE + reset_done's restart"
    else:
        assert seen.get("term") and seen.get("rewarded"), seen
        # a pool restart happens BEFORE the next step: the one that follows the last step's close is still pending
        assert torch.equal(stats.counts[:, 0], env.episode - e0 + stats.over.to(torch.int32))
        assert all(c[1] == BEFORE for c in be.calls if c[0] == "stats")
    s = stats.summary()
    n = int(want["counts"][:, 0].sum())
    assert s["episodes"] == n and s["aborted"] == 0
    assert s["mean_length"] == want["sum_length"].sum() / n
    assert s["mean_return"] == pytest.approx((want["sum_return"].sum(0) / n).tolist(), rel=1e-12)
    assert s["terminated"] == want["counts"][:, 1].sum() / n and s["rewarded"] == want["counts"][:, 2].sum() / n


def test_explicit_reset_done_loop_skips_the_steps_past_the_end():
    env = make_env("plain", backend=StatsOracle(SPEC))
    stats = env.track_episodes()
    B, A, T = env.batch, SPEC.num_agents, 4 * SPEC.max_steps + 3
    acts = actions_for(B, A, T, 2)
    want, seen = new_state(B, A), {}
    for t in range(T):
        env.step(acts[t])
        r, te, tr, _ = record(env)
        model_stats(want, r, te, tr, None, NONE, seen=seen)
        if t % 3 == 2:                                    # (finished envs wait up to two steps for their restart)
            model_restart(want, env.reset_done().numpy().copy(), seen)
    assert_same(snapshot(stats), want)
    assert seen.get("skipped") and seen.get("trunc") and seen.get("term") and not seen.get("abort"), seen


def test_reset_of_chosen_envs_aborts_their_running_episodes():
    env = make_env("gen", backend=StatsOracle(SPEC))
    stats = env.track_episodes()
    B, A = env.batch, SPEC.num_agents
    acts = actions_for(B, A, 2, 3)
    env.step(acts[0], auto_reset=True); env.step(acts[1], auto_reset=True)
    before = snapshot(stats)
    mask = torch.tensor([1, 1, 0, 0, 1, 0, 1], dtype=torch.bool)
    env.reset(seed=5, mask=mask)
    running = mask.numpy() & (before["cur_length"] > 0) & (before["over"] == 0)
    assert running.sum() >= 2
    got = snapshot(stats)
    assert (got["counts"][:, 3] == running.astype(np.int32)).all() and int(got["counts"][:, 3].sum()) == int(running.sum())
    assert not got["cur_length"][mask.numpy()].any() and not got["cur_return"][mask.numpy()].any()
    assert (got["cur_length"][~mask.numpy()] == before["cur_length"][~mask.numpy()]).all()
    want = {k: v.copy() for k, v in before.items()}
    model_restart(want, mask.numpy())
    assert_same(got, want)
    # load_state: every env restarts, and one that is already over stays out of the books
    sd = env.state_dict()
    sd["step_count"][1] = SPEC.max_steps
    env.load_state(sd["grid"], sd["agents"], sd["rng"], sd["aux"], sd["step_count"])
    got = snapshot(stats)
    assert got["over"].tolist() == [0, 1, 0, 0, 0, 0, 0] and not got["cur_length"].any()


def test_enabling_mid_run_skips_the_envs_that_are_already_over():
    env = make_env("plain", backend=StatsOracle(SPEC))
    B, A = env.batch, SPEC.num_agents
    acts = actions_for(B, A, 8, 4)
    for t in range(4):
        env.step(acts[t])
    done = env.is_done().numpy().copy()
    assert done.any()
    stats = env.track_episodes()
    assert stats.over.numpy().astype(bool).tolist() == done.tolist()
    want = new_state(B, A)
    want["over"][:] = done
    env.step(acts[4])
    model_stats(want, *record(env)[:3], None, NONE)
    assert_same(snapshot(stats), want)
    assert not snapshot(stats)["cur_length"][done].any() and not snapshot(stats)["counts"][done].any()
    assert env.track_episodes(None) is None and env.episode_stats is None
    env.step(acts[5])                                     # ... and steps on untracked


@pytest.mark.parametrize("form,trace", [("pool", True), ("gen", True), ("plain", False), ("pool", False)])
def test_rollout_is_one_call_over_its_outputs(form, trace):
    be = StatsOracle(SPEC)
    env = make_env(form, backend=be)
    ref = make_env(form, backend=StatsOracle(SPEC))
    stats, rstats = env.track_episodes(trace=trace), ref.track_episodes()
    B, A, T = env.batch, SPEC.num_agents, 2 * SPEC.max_steps + 3
    acts = actions_for(B, A, T, 5)
    ar = form != "plain"
    be.calls.clear()
    out = env.rollout(acts, auto_reset=ar)
    assert be.calls == [("stats", {"pool": BEFORE, "gen": AFTER, "plain": NONE}[form], T)]
    want = new_state(B, A)
    tr = new_trace(T, B, A)
    model_stats(want, out["reward"].numpy(), out["terminated"].numpy(), out["truncated"].numpy(),
                out["was_reset"].numpy() if ar else None, {"pool": BEFORE, "gen": AFTER, "plain": NONE}[form], tr)
    assert_same(snapshot(stats), want, form)
    for t in range(T):                                    # ... which is what the same steps give one by one
        ref.step(acts[t], auto_reset=ar)
    assert_same(snapshot(rstats), want, form + " steps")
    if trace:
        for k, name in zip(TRACE, ("episode_closed", "episode_return", "episode_length")):
            assert out[name].numpy().tobytes() == tr[k].tobytes(), name
        assert out["episode_closed"].any()
    else:
        assert "episode_closed" not in out


def test_sub_shards_account_for_their_slices():
    spec, B = SPEC, 130
    env = make_env("pool", B=B, backend=StatsOracle(spec))
    ref = make_env("pool", B=B, backend=StatsOracle(spec))
    stale = env.split(2)
    stats, rstats = env.track_episodes(), ref.track_episodes()
    with pytest.raises(RuntimeError, match="track_episodes"):
        stale[0].step(torch.zeros((stale[0].batch, 2), dtype=torch.int8), auto_reset=True)
    shards = env.split(2)
    assert len(shards) == 2 and sum(s.batch for s in shards) == B
    acts = actions_for(B, 2, 6, 6)
    for t in range(6):
        ref.step(acts[t], auto_reset=True)
    for sh in shards:                                                      # one chain after the other: envs are independent
        lo, hi = sh._range
        assert sh.episode_stats.cur_return.data_ptr() == stats.cur_return[lo:hi].data_ptr()
        for t in range(6):
            sh.step(acts[t, lo:hi], auto_reset=True)
    assert_same(snapshot(stats), snapshot(rstats))
    assert int(stats.counts[:, 0].sum()) > 0


def test_totals_checkpoint_and_the_two_refusals():
    env = make_env("pool", B=130, backend=StatsOracle(SPEC))
    stats = env.track_episodes()
    acts = actions_for(130, 2, 6, 7)
    for t in range(6):
        env.step(acts[t], auto_reset=True)
    keys = set(env.state_dict())
    sd = stats.state_dict()
    assert set(sd) == set(NAMES) and "episode_stats" not in keys and keys == set(make_env("pool", B=130, backend=StatsOracle(SPEC)).state_dict())
    running = snapshot(stats)
    assert running["counts"][:, 0].any() and running["cur_length"].any()
    stats.reset_totals()
    got = snapshot(stats)
    assert not got["sum_return"].any() and not got["sum_length"].any() and not got["counts"].any()
    for n in ("cur_return", "cur_length", "over", "last_return", "last_length"):
        assert got[n].tobytes() == running[n].tobytes(), n
    assert stats.summary()["episodes"] == 0
    other = EpisodeStats(130, 2, "cpu")
    other.load_state_dict(sd)
    assert_same(snapshot(other), running)
    with pytest.raises(ValueError, match="cur_return"):
        EpisodeStats(4, 2, "cpu").load_state_dict(sd)
    with pytest.raises(RuntimeError, match="track_episodes"):
        env.persistent(max_steps=4)
    with pytest.raises(RuntimeError, match="track_episodes"):
        env.step(acts[0], sub_shards=2)
    env.track_episodes(None)
    with pytest.raises(RuntimeError, match="HIP backend"):       # (tracking off: what an oracle-backed env always answered)
        env.persistent(max_steps=4)


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------------

def test_c_abi_argument_validation():
    L = _lib.lib()
    INV, UNS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
    assert L.mgx_abi_version() == 11
    p = 4096                                              # (never dereferenced: every call returns before a launch)
    sc = EnvSpec(5, 5, 2, 3, max_steps=4).to_c()
    full = lambda **kw: _lib.MgxEpisodeStats(*[kw.get(n, p) for n in NAMES])
    S = lambda sc_, B, T, rew, te, tr, wr, mode, st, trace=None: L.mgx_episode_stats(
        C.byref(sc_) if sc_ else None, B, T, rew, te, tr, wr, mode, C.byref(st) if st else None,
        C.byref(trace) if trace else None, None)
    R = lambda sc_, B, sel, st: L.mgx_episode_restart(C.byref(sc_) if sc_ else None, B, sel, C.byref(st) if st else None, None)
    st = full()
    # the spec check comes first
    assert S(None, 4, 1, p, p, p, p, NONE, st) == INV and R(None, 4, None, st) == INV
    bad = EnvSpec(5, 5, 2, 3).to_c()
    for n in (0, 33):
        bad.num_agents = n
        assert S(bad, 0, 0, None, None, None, None, NONE, None) == INV and R(bad, 0, None, None) == INV
    assert S(sc, -1, 1, p, p, p, p, NONE, st) == INV and R(sc, -1, None, st) == INV
    assert S(sc, 4, -1, p, p, p, p, NONE, st) == INV
    # nothing to do: MGX_OK, whatever the tensors
    assert S(sc, 0, 1, None, None, None, None, NONE, None) == 0 and S(sc, 4, 0, None, None, None, None, NONE, None) == 0
    assert S(sc, 0, 0, None, None, None, None, BEFORE, None) == 0 and R(sc, 0, None, None) == 0
    # a missing required pointer
    assert S(sc, 4, 1, None, p, p, p, NONE, st) == INV and S(sc, 4, 1, p, None, p, p, NONE, st) == INV
    assert S(sc, 4, 1, p, p, None, p, NONE, st) == INV and S(sc, 4, 1, p, p, p, p, NONE, None) == INV and R(sc, 4, None, None) == INV
    for n in NAMES:
        assert S(sc, 4, 1, p, p, p, p, NONE, full(**{n: None})) == INV, n
        assert R(sc, 4, None, full(**{n: None})) == INV, n
    # the restart modes
    for mode in (BEFORE, AFTER):
        assert S(sc, 4, 1, p, p, p, None, mode, st) == INV
    for mode in (-1, 3):
        assert S(sc, 4, 1, p, p, p, p, mode, st) == INV
    # alignment: 8 bytes for f64 / i64, 4 for i32
    assert S(sc, 4, 1, p + 4, p, p, p, NONE, st) == INV
    for n in ("cur_return", "last_return", "sum_return", "sum_length"):
        assert S(sc, 4, 1, p, p, p, p, NONE, full(**{n: p + 4})) == INV and R(sc, 4, None, full(**{n: p + 4})) == INV, n
    for n in ("cur_length", "last_length", "counts"):
        assert S(sc, 4, 1, p, p, p, p, NONE, full(**{n: p + 2})) == INV and R(sc, 4, None, full(**{n: p + 2})) == INV, n
    assert S(sc, 4, 1, p, p, p, p, NONE, st, _lib.MgxEpisodeTrace(p, p + 4, p)) == INV
    assert S(sc, 4, 1, p, p, p, p, NONE, st, _lib.MgxEpisodeTrace(p, p, p + 2)) == INV
    # more wavefronts than a grid holds: one per 64 / A envs (A = 32: two envs), the restart one per 64 envs
    wide = EnvSpec(5, 5, 32, 3).to_c()
    assert S(wide, 2 * (2 ** 31 - 1) + 1, 1, p, p, p, p, NONE, st) == UNS
    assert R(sc, 64 * (2 ** 31 - 1) + 1, None, st) == UNS
    assert S(sc, 32 * (2 ** 31 - 1) + 1, 1, p, p, p, p, NONE, st) == UNS


def test_the_exports_are_the_headers_declarations():
    from tests.test_capi import declared_functions
    names = declared_functions()
    assert {"mgx_episode_stats", "mgx_episode_restart"} <= set(names) and set(names) == set(_lib.EXPORTS)
    L = _lib.lib()
    assert L.mgx_episode_stats is not None and L.mgx_episode_restart is not None
    assert L.mgx_abi_version() == _lib.ABI_VERSION == 11


def test_the_ctypes_structs_match_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mgx.h"', 'int main(void) {']
    structs = {"MgxEpisodeStats": _lib.MgxEpisodeStats, "MgxEpisodeTrace": _lib.MgxEpisodeTrace}
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f}));' for f, _ in cls._fields_]
        lines.append('  printf("\\n");')
    lines += ['  printf("modes %d %d %d\\n", MGX_RESTART_NONE, MGX_RESTART_BEFORE, MGX_RESTART_AFTER);', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call([cc, "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    for line, (name, cls) in zip(out, structs.items()):
        want = [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
        assert line.split() == [name] + [str(v) for v in want], line
    assert out[-1].split() == ["modes", str(NONE), str(BEFORE), str(AFTER)]
