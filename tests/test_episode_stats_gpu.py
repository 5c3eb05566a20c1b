"""Episode accounting on the GPU: episode_stats_kernel / episode_restart_kernel (csrc/mgx_stats.hip) against the sequential NumPy
model of tests/test_episode_stats.py, bit for bit -- first on raw synthetic tensors through the C ABI at the edges of the kernel's
mapping (a wavefront owns G = 64 // A whole envs), then through BatchedMultiGridEnv.track_episodes() on small real envs, where the
recorded outputs of every step are fed to the model."""
import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec
from tests.test_episode_stats import (AFTER, BEFORE, NAMES, NONE, SPEC, TRACE, actions_for, assert_same, make_env, model_restart,
                                      model_stats, new_state, new_trace, record, snapshot)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def backend(A):
    from multigrid_amd.ops import HipBackend
    return HipBackend(EnvSpec(5, 5, A, 3), torch.device(DEV))


def to_dev(d):
    return {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}


def synthetic(B, A, T, seed):
    """Step outputs as no engine would order them, per env: closes by truncation, by termination and by both; steps with some but not
    all agents terminated; stretches that report every agent terminated without a restart (the LockedHallway shape); restarts of
    running episodes, of closed ones, and two in a row (length 0).  Rewards over sixteen decades, either sign: their sums depend on
    the order."""
    r = np.random.default_rng(seed)
    reward = r.standard_normal((T, B, A)) * 10.0 ** r.integers(-8, 9, size=(T, B, A))
    reward[r.random((T, B, A)) < 0.2] = 0.0
    truncated = (r.random((T, B)) < 0.15).astype(np.uint8)
    terminated = (r.random((T, B, A)) < 0.25).astype(np.uint8) * r.integers(1, 256, size=(T, B, A)).astype(np.uint8)
    terminated[r.random((T, B)) < 0.15] = 1
    was_reset = (r.random((T, B)) < 0.25).astype(np.uint8) * r.integers(1, 256, size=(T, B)).astype(np.uint8)
    stretch = np.arange(B) % 4 == 0                      # env 0, 4, ...: reported terminated at t = 2, left alone for the next two
    if T >= 5:
        terminated[2:5, stretch] = 1
        was_reset[2:5, stretch] = 0
    return reward, terminated, truncated, was_reset


def call(be, B, st, inp, t0, t1, mode, trace=None):
    reward, terminated, truncated, was_reset = (x[t0:t1].contiguous() for x in inp)
    be.episode_stats(B, t1 - t0, reward, terminated, truncated, was_reset if mode != NONE else None, mode, st, trace)


@pytest.mark.parametrize("mode", [NONE, BEFORE, AFTER], ids=["none", "before", "after"])
@pytest.mark.parametrize("A", [1, 2, 3, 5, 32])
def test_kernel_equals_the_model_at_the_mapping_edges(A, mode):
    G = 64 // A
    be = backend(A)
    seen = {}
    for B in sorted({1, G - 1, G, G + 1, 4 * G, 4 * G + 1} - {0}):
        T = 10                                            # a call of 1 step, one of 2, one of 7
        inp = synthetic(B, A, T, 1000 * A + 10 * B + mode)
        dinp = [torch.from_numpy(x).to(DEV) for x in inp]
        want = new_state(B, A)
        got = to_dev(want)
        ctx = f"A={A} B={B} mode={mode}"
        # T = 1, no trace
        model_stats(want, *(x[0:1] for x in inp), mode, seen=seen)
        call(be, B, got, dinp, 0, 1, mode)
        assert_same({n: got[n].cpu().numpy() for n in NAMES}, want, ctx + " T=1")
        # T = 2, one trace pointer at a time
        keep = TRACE[B % 3]
        tr = {k: v for k, v in new_trace(2, B, A).items() if k == keep}
        dtr = to_dev(tr)
        model_stats(want, *(x[1:3] for x in inp), mode, trace=tr, seen=seen)
        call(be, B, got, dinp, 1, 3, mode, trace=dtr)
        assert_same({n: got[n].cpu().numpy() for n in NAMES}, want, ctx + " T=2")
        assert dtr[keep].cpu().numpy().tobytes() == tr[keep].tobytes(), ctx + " trace " + keep
        # T = 7, the whole trace; and the same seven steps one call each
        singles = {n: t.clone() for n, t in got.items()}
        tr = new_trace(7, B, A)
        dtr = to_dev(tr)
        model_stats(want, *(x[3:10] for x in inp), mode, trace=tr, seen=seen)
        call(be, B, got, dinp, 3, 10, mode, trace=dtr)
        assert_same({n: got[n].cpu().numpy() for n in NAMES}, want, ctx + " T=7")
        for k in TRACE:
            assert dtr[k].cpu().numpy().tobytes() == tr[k].tobytes(), ctx + " trace " + k
        for t in range(3, 10):
            call(be, B, singles, dinp, t, t + 1, mode)
        assert_same({n: singles[n].cpu().numpy() for n in NAMES}, want, ctx + " 7 x T=1")
    # the inputs reach every clause of the rule (or the comparison above shows nothing)
    need = ["trunc", "term", "both", "rewarded", "skipped"] + (["partial_term"] if A > 1 else []) \
        + (["abort"] if mode != NONE else []) + (["restart_at_0"] if mode == BEFORE else [])     # (AFTER follows a counted step)
    assert all(seen.get(k) for k in need), (need, seen)


@pytest.mark.parametrize("A", [2, 5])
def test_restart_operation(A):
    G = 64 // A
    B = 4 * G + 1
    be = backend(A)
    inp = synthetic(B, A, 3, 7 + A)
    inp[1][:, B - 1], inp[2][:, B - 1] = 0, 0             # (the last env's episode is still running)
    want = new_state(B, A)
    model_stats(want, *inp, NONE)
    assert (want["cur_length"] > 0).sum() > 2 and want["over"].any() and want["cur_length"][B - 1] > 0
    got = to_dev(new_state(B, A))
    call(be, B, got, [torch.from_numpy(x).to(DEV) for x in inp], 0, 3, NONE)
    host = lambda: {n: got[n].cpu().numpy() for n in NAMES}
    assert_same(host(), want, "before the restarts")
    be.episode_restart(B, torch.zeros(B, dtype=torch.uint8, device=DEV), got)          # nobody: nothing changes, byte for byte
    assert_same(host(), want, "all-zero select")
    last = np.zeros(B, np.uint8)
    last[B - 1] = 7
    model_restart(want, last)
    be.episode_restart(B, torch.from_numpy(last).to(DEV), got)                         # only the last env
    assert_same(host(), want, "the last env")
    assert want["counts"][B - 1, 3] == 1 and want["counts"][:, 3].sum() == 1
    seen = model_restart(want, None)
    be.episode_restart(B, None, got)                                                   # everybody
    assert_same(host(), want, "select = NULL")
    assert seen.get("abort") and not want["over"].any() and not want["cur_length"].any()


# ---- through the env ------------------------------------------------------------------------------------------------------------------

def gen_env(spec, kind, B, **kw):
    env = BatchedMultiGridEnv(spec, B, DEV)
    env.set_layout_generator(kind, layout_seed=5, staged=False, **kw)
    env.reset(seed=3)
    return env


CASES = {
    "empty5_a2_pool": lambda B: make_env("pool", B=B, dev=DEV),
    "emptyrandom5_a6_gen": lambda B: gen_env(EnvSpec(5, 5, 6, 7, max_steps=3), "empty_random", B),
    "bup_rs5_a2_gen": lambda B: gen_env(EnvSpec(9, 5, 2, 7, max_steps=5, joint_reward=True, env_kind="blockedunlockpickup"),
                                        "blockedunlockpickup", B, room_size=5),
    "lockedhallway_13x9_a2_gen": lambda B: gen_env(EnvSpec(13, 9, 2, 7, max_steps=4, joint_reward=True, env_kind="lockedhallway"),
                                                   "lockedhallway", B, room_size=5),
}


@pytest.mark.parametrize("B", [130, 515])
@pytest.mark.parametrize("case", list(CASES))
def test_tracked_env_under_auto_reset(case, B):
    env = CASES[case](B)
    sp, A = env.spec, env.spec.num_agents
    pool = case.endswith("_pool")
    stats = env.track_episodes()
    e0 = env.episode.clone()
    T = 4 * sp.max_steps + 3
    acts = actions_for(B, A, T, 11).to(DEV)
    want, seen = new_state(B, A), {}
    trunc_lengths = []
    for t in range(T):
        env.step(acts[t], auto_reset=True)
        r, te, tr, wr = record(env)
        before = want["counts"][:, 0].copy()
        model_stats(want, r, te, tr, wr, BEFORE if pool else AFTER, seen=seen)
        closed = want["counts"][:, 0] > before
        trunc_lengths.append(want["last_length"][closed & (tr != 0)])
        assert (want["last_length"][closed] <= sp.max_steps).all()
    env.check_errors()
    got = snapshot(stats)
    assert_same(got, want, case)
    # what does not come from the model
    assert not got["counts"][:, 3].any(), "auto-reset alone aborts nothing: the outputs' ends and the engine's restarts line up"
    episodes = (env.episode - e0).cpu().numpy()
    if pool:        # the pool restart comes BEFORE the next step: the one that answers the last step's close is still pending
        assert (got["counts"][:, 0] == episodes + got["over"]).all()
    else:           # the generator restarts right AFTER the closing step: none pending
        assert (got["counts"][:, 0] == episodes).all() and not got["over"].any()
    assert (got["last_length"] <= sp.max_steps).all() and got["counts"][:, 0].min() >= 3
    assert len(np.concatenate(trunc_lengths)) and (np.concatenate(trunc_lengths) == sp.max_steps).all()
    if pool:
        assert got["counts"][:, 1].sum() > 0 and got["counts"][:, 2].sum() > 0, "the case that closes episodes by termination"
    s = stats.summary()
    assert s["episodes"] == int(got["counts"][:, 0].sum()) and s["aborted"] == 0
    assert s["mean_length"] == got["sum_length"].sum() / s["episodes"]


def test_every_stepping_form_gives_the_same_books():
    B, A, T = 130, SPEC.num_agents, 2 * SPEC.max_steps + 3
    acts = actions_for(B, A, T, 12).to(DEV)
    books = {}
    env = make_env("pool", B=B, dev=DEV)
    stats = env.track_episodes()
    for t in range(T):
        env.step(acts[t], auto_reset=True)
    books["step"] = snapshot(stats)
    assert books["step"]["counts"][:, 0].sum() > B
    env = make_env("pool", B=B, dev=DEV)
    stats = env.track_episodes(trace=True)
    out = env.rollout(acts, auto_reset=True)
    books["rollout"] = snapshot(stats)
    want, tr = new_state(B, A), new_trace(T, B, A)
    model_stats(want, *(out[k].cpu().numpy() for k in ("reward", "terminated", "truncated", "was_reset")), BEFORE, trace=tr)
    assert_same(books["rollout"], want, "rollout against the model")
    for k, name in zip(TRACE, ("episode_closed", "episode_return", "episode_length")):
        assert out[name].cpu().numpy().tobytes() == tr[k].tobytes(), name
    for name, shards in (("graph", 1), ("graph of two sub-shards", 2)):
        env = make_env("pool", B=B, dev=DEV)
        stats = env.track_episodes()
        g = env.capture_steps(acts, auto_reset=True, sub_shards=shards)
        assert g.sub_shards == shards
        if shards == 1:
            with pytest.raises(RuntimeError, match="captured before"):
                env.track_episodes(None)
                g.replay()
            stats = env.track_episodes()
            g = env.capture_steps(acts, auto_reset=True)
        g.replay()
        torch.cuda.synchronize()
        books[name] = snapshot(stats)
    for name, b in books.items():
        assert_same(b, books["step"], name)


def test_explicit_resets():
    B, A = 130, SPEC.num_agents
    env = make_env("plain", B=B, dev=DEV)
    stats = env.track_episodes()
    T = 4 * SPEC.max_steps + 3
    acts = actions_for(B, A, T, 13).to(DEV)
    want, seen = new_state(B, A), {}
    for t in range(T):
        env.step(acts[t])
        r, te, tr, _ = record(env)
        model_stats(want, r, te, tr, None, NONE, seen=seen)
        if t % 3 == 2:                                    # (finished envs wait up to two steps for their restart: steps past the end)
            model_restart(want, env.reset_done().cpu().numpy(), seen)
    assert_same(snapshot(stats), want, "reset_done loop")
    assert seen.get("skipped") and seen.get("trunc") and seen.get("term") and not seen.get("abort"), seen
    env.step(acts[0]); env.step(acts[1])
    before = snapshot(stats)
    mask = torch.arange(B, device=DEV) % 3 != 1
    env.reset(seed=9, mask=mask)
    running = mask.cpu().numpy() & (before["cur_length"] > 0) & (before["over"] == 0)
    got = snapshot(stats)
    assert running.sum() > 10 and int((got["counts"][:, 3] - before["counts"][:, 3]).sum()) == int(running.sum())
    assert ((got["counts"][:, 3] - before["counts"][:, 3]) == running).all()
    want = {k: v.copy() for k, v in before.items()}
    model_restart(want, mask.cpu().numpy())
    assert_same(got, want, "reset(seed, mask)")


def test_an_untracked_env_steps_exactly_as_a_tracked_one():
    """The composite launcher must not disturb the step, and an env that never tracked is the env of before."""
    B, A, T = 130, SPEC.num_agents, 2 * SPEC.max_steps + 3
    acts = actions_for(B, A, T, 14).to(DEV)
    plain, tracked = make_env("pool", B=B, dev=DEV), make_env("pool", B=B, dev=DEV)
    tracked.track_episodes()
    assert plain.episode_stats is None
    for t in range(T):
        a, b = plain.step(acts[t], auto_reset=True), tracked.step(acts[t], auto_reset=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    for k in ("_cells", "agents", "rng", "step_count", "aux", "episode", "was_reset", "_marker"):
        assert torch.equal(getattr(plain, k), getattr(tracked, k)), k
    assert plain._bound[(True, False)][0].__name__ == "step" and tracked._bound[(True, False)][0].__name__ == "tracked_step"
