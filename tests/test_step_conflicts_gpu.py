"""Every step-kernel family on the constructed conflict corpus (tests/golden/conflict_*.npz, oracle/gen_golden.py: record_conflicts):
envs in which the visiting order decides the outcome -- two agents at one key, a door closed in front of a walking agent, a drop
into the cell another agent steps into, an episode-ending event ahead of an agent that still had something to do -- compared with
the REFERENCE's recorded bytes.  tests/test_step_path_census.py counts which of the kernel's decisions (cell conflict, fallback,
commit cutoff, event cutoff) each file reaches; tests/test_rules_host.py replays the same files through the host build of
mgx_rules.h in both fallback commits.  What is left to this file is the kernels' own plumbing around those rules: the LDS exchange
of the written offsets and of the visiting order, the ballots and their per-env masks at every env slot of a wavefront (the batch
sizes are odd and no multiple of any envs-per-wavefront, so under Fixture.rep every scenario meets every slot, the last one and
ragged last wavefronts included), and P1c's pickup of where the loop starts.

Helpers and the family list are those of tests/test_reference_random_states_gpu.py."""
import contextlib
import os

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, _lib
from oracle import binding as ob
from tests import test_reference_random_states_gpu as R
from tests import util

pytestmark = pytest.mark.gpu
DEV = R.DEV
FIX = dict(zip(util.CONFLICT_IDS, util.CONFLICT_GOLDEN))
C24 = "conflict_16x16_a4_v7"
C5 = "conflict_64x64_a16_v9"
A16 = "conflict_20x14_a16_v9"
BUP = "conflict_bup_11x6_a2_v7"
OUTS = ("obs", "dir", "reward", "terminated", "truncated")
_FIXTURES = {}


def fixture(name) -> R.Fixture:
    if name not in _FIXTURES:
        _FIXTURES[name] = R.Fixture(name, FIX[name])
    return _FIXTURES[name]


def test_the_corpus_is_complete():
    assert {C24, C5, A16, BUP, "conflict_9x6_a2_v5", "conflict_10x8_a3_v7", "conflict_13x10_a5_v9",
            "conflict_10x8_a3_v7_boxes"} <= set(FIX)
    for name in FIX:
        fx = fixture(name)
        per_wave = {_lib.launch_info(fx.spec, n)["envs_per_wavefront"] for n in (fx.B, 3 * fx.B + 5, 1 << 16)}
        assert fx.B % 2 == 1 and all(fx.B % g for g in per_wave if g > 1), (name, fx.B, per_wave)
    assert fixture("conflict_10x8_a3_v7_boxes").filled_boxes and not fixture(C5).filled_boxes


@pytest.mark.parametrize("name", util.CONFLICT_IDS)
def test_latency_family(name):
    fx = fixture(name)
    for N in (fx.B, 3 * fx.B + 5):
        env = fx.env(N)
        assert R.waves(env.spec, N) <= 2048
        obs, dr = env.gen_obs()
        R._same(obs, fx.dev("obs0"), fx.B, f"{name} N={N} gen_obs", "obs")
        R._same(dr, fx.dev("dir0"), fx.B, f"{name} N={N} gen_obs", "dir")
        R.run_steps(fx, env, f"{name} latency N={N}")


@pytest.mark.parametrize("name", util.CONFLICT_IDS)
def test_throughput_family(name):
    fx = fixture(name)
    gw = _lib.launch_info(fx.spec, 1 << 16)["envs_per_wavefront"]
    N = 2049 * gw + 3
    env = fx.env(N)
    assert R.waves(env.spec, N) > 2048
    R.run_steps(fx, env, f"{name} throughput N={N}")


@pytest.mark.parametrize("name", util.CONFLICT_IDS)
def test_one_hot_family(name):
    fx = fixture(name)
    N = 2 * fx.B + 7
    R.run_steps(fx, fx.env(N), f"{name} one-hot", one_hot=True)
    if fx.spec.env_kind == "empty" and not fx.filled_boxes:
        R.run_steps(fx, fx.env(N, cell_bytes=1), f"{name} compact one-hot", one_hot=True)


@pytest.mark.parametrize("name", util.CONFLICT_IDS)
def test_compact_and_byte_grid_families(name):
    """cell_bytes = 1 and 3; the byte-grid commit writes the grid at (off >> 1) * 3, a path of its own."""
    fx = fixture(name)
    N = 2 * fx.B + 3
    if fx.filled_boxes:
        with pytest.raises(ValueError, match="compact"):
            fx.env(N, cell_bytes=1)
    else:
        R.run_steps(fx, fx.env(N, cell_bytes=1), f"{name} compact")
    R.run_steps(fx, fx.env(N, cell_bytes=3), f"{name} byte grid")


def _check_rollout(fx, env, out, ctx):
    for t in range(fx.T):
        R.check_outputs(fx, t, [out[k][t] for k in OUTS], f"{ctx} step {t}")
    R.check_state(fx, env, fx.T - 1, ctx)
    env.check_errors()


@pytest.mark.parametrize("name", util.CONFLICT_IDS)
def test_rollout_family(name):
    fx = fixture(name)
    N = 2 * fx.B + 9
    env = fx.env(N)
    _check_rollout(fx, env, env.rollout(fx.actions(N)), f"{name} rollout")


# (fixture, batch, cell_bytes, kShapes entry of the plain step): the batches of test_reference_random_states_gpu.SHAPED
SHAPED = [(C24, 4096, 2, 1), (C24, 16384, 2, 2), (BUP, 16384, 2, 3), (C5, 32768, 2, 4), (C5, 36864, 1, 5), (C5, 32768, 1, 6)]
assert [s[1:] for s in SHAPED] == [s[1:] for s in R.SHAPED]


@pytest.mark.parametrize("name,N,cb,shape", SHAPED, ids=[f"shape{s[3]}" for s in SHAPED])
def test_shape_specialised_family(name, N, cb, shape):
    fx = fixture(name)
    env = fx.env(N, cell_bytes=cb)
    assert _lib.launch_info(env.spec, N)["fixed_shape"] == shape
    R.run_steps(fx, env, f"{name} shape {shape}")
    del env
    torch.cuda.empty_cache()


def test_specialise_family():
    fx = fixture("conflict_10x8_a3_v7")
    N = 3 * fx.B + 1
    env = fx.env(N)
    assert env.specialise() in ("compiled", "registered")
    R.run_steps(fx, env, "specialise()")


def test_resident_rollout_family():
    fx = fixture(C24)
    for ns in (1, 2, 9):
        for N in (fx.B + 5, 3 * fx.B + 21):
            env = fx.env(N)
            with R.resident(ns):
                assert _lib.launch_info(env.spec, N, roll=True)["resident_shape"] == {1: 7, 2: 8, 9: 9}[ns]
                out = env.rollout(fx.actions(N))
            _check_rollout(fx, env, out, f"resident ns={ns} N={N}")


@pytest.mark.parametrize("ns", [0, 1, 2])
def test_persistent_family(ns):
    fx = fixture(C24)
    N = 2 * fx.B + 11
    env = fx.env(N)
    with R.resident(ns) if ns else contextlib.nullcontext():
        with env.persistent(max_steps=fx.T) as ps:
            for t in range(fx.T):
                R.check_outputs(fx, t, ps.step(fx.actions(N, t)), f"persistent ns={ns} step {t}")
    assert ps.timeouts == 0 and ps.steps_completed == fx.T
    R.check_state(fx, env, fx.T - 1, f"persistent ns={ns}")
    env.check_errors()


@pytest.mark.parametrize("name", [C24, "conflict_9x6_a2_v5", BUP])
def test_sub_shard_chains(name):
    fx = fixture(name)
    N = 8 * fx.B + 64
    for P in (2, 3):
        env = fx.env(N)
        g = env.capture_steps(fx.actions(N), sub_shards=P)
        assert g.sub_shards == P
        g.replay()
        torch.cuda.synchronize()
        t = fx.T - 1
        R.check_outputs(fx, t, (env.obs, env.dir, env.reward, env.terminated, env.truncated), f"{name} graph P={P}")
        R.check_state(fx, env, t, f"{name} graph P={P}")
        env = fx.env(N)
        for t in range(fx.T):
            env.step(fx.actions(N, t), sub_shards=P)
            env.join()
            R.check_outputs(fx, t, (env.obs, env.dir, env.reward, env.terminated, env.truncated), f"{name} eager P={P} step {t}")
        R.check_state(fx, env, fx.T - 1, f"{name} eager P={P}")
        env.check_errors()


# --------------------------------------------------------------------------------------------------------- mixed wavefronts

def _load(spec, grid, agents, rng, aux, step_count):
    env = BatchedMultiGridEnv(spec, grid.shape[0], DEV)
    env.load_state(grid, agents, rng, aux if spec.env_kind != "empty" else None, step_count, validate=False)
    return env


def _compare(env, outs, want, envs, ctx):
    """outputs and state of the launch against the numpy arrays of `want`, on the envs of the index array `envs`"""
    got = dict(zip(OUTS, (o.cpu().numpy() for o in outs[:5])))
    got.update(grid=env.grid.cpu().numpy(), agents=env.agents.cpu().numpy(), rng=env.rng.cpu().numpy().view(np.uint64),
               step_count=env.step_count.cpu().numpy())
    for k, w in want.items():
        if k == "rng" and env.spec.num_agents == 1:
            continue
        g = got[k][envs]
        w = np.asarray(w)[envs]
        if k == "reward":
            g, w = g.view(np.int64), w.view(np.int64)
        bad = np.nonzero((g.reshape(len(envs), -1) != w.reshape(len(envs), -1)).any(-1))[0]
        assert len(bad) == 0, f"{ctx}: {k} differs in envs {envs[bad][:6].tolist()}"


@pytest.mark.parametrize("name", util.CONFLICT_IDS)
def test_mixed_wavefronts(name):
    """Conflict envs alternating with untouched random_state envs of the same spec: the fallback mask of a wavefront is sparse, and
    the written offsets are exchanged in wavefronts whose other envs write nothing.  Expected: the reference's bytes for the conflict
    envs, the oracle for the others."""
    fx = fixture(name)
    z, spec, B = fx.z, fx.spec, fx.B
    N = 2 * B
    st = util.random_state(spec, B, seed=4242 + B, box_contents_p=0.5 if fx.filled_boxes else 0.0)
    if spec.env_kind == "empty":
        st["target"][:] = 0

    def mix(a, b):
        out = np.empty((N,) + a.shape[1:], a.dtype)
        out[0::2], out[1::2] = a, b
        return out

    env = _load(spec, mix(z["grid0"], st["grid"]), mix(z["agents0"], st["agents"]), mix(z["rng0"], st["rng"]),
                mix(z["aux"], st["target"]), mix(z["step_count0"], st["step_count"]))
    sd = spec.as_dict()
    every = np.arange(N)
    for t in range(fx.T):
        act = util.random_actions(B, spec.num_agents, seed=77 + t)
        o, d, r, te, tr = ob.step_batch(sd, st["grid"], st["agents"], st["rng"], st["step_count"], act, st["target"])
        outs = env.step(torch.from_numpy(mix(z["actions"][t], act)).to(DEV))
        want = dict(obs=mix(z["obs"][t], o), dir=mix(z["dir"][t], d), reward=mix(z["reward"][t], r),
                    terminated=mix(z["terminated"][t], te), truncated=mix(z["truncated"][t], tr),
                    grid=mix(z["grid"][t], st["grid"]), agents=mix(z["agents"][t], st["agents"]), rng=mix(z["rng"][t], st["rng"]),
                    step_count=mix(z["step_count0"] + (t + 1), st["step_count"]))
        _compare(env, outs, want, every, f"{name} mixed step {t}")
    env.check_errors()


# ------------------------------------------------------------------------------------------------ unknown actions, contended

@pytest.mark.parametrize("name", util.CONFLICT_IDS)
def test_unknown_action_in_a_contended_env(name):
    """The reference raises on an unknown action (base.py:473-474), so nothing of it can be recorded: the oracle is the comparison.
    Three envs in four get action 7 for ONE agent -- the one the recorded visiting order visits first, in the middle, last.  The
    device's error words must count exactly the envs in which the oracle raises and name the lowest; every other env's outputs and
    state must be the oracle's."""
    fx = fixture(name)
    z, spec, B, A = fx.z, fx.spec, fx.B, fx.spec.num_agents
    act = z["actions"][0].copy()
    for b in range(B):
        if b % 4:
            act[b, int(z["order"][0, b][{1: 0, 2: A // 2, 3: A - 1}[b % 4]])] = 7
    st = {k: z[k + "0"].copy() for k in ("grid", "agents", "rng", "step_count")}
    aux = z["aux"].copy()
    sd = spec.as_dict()
    v = spec.view_size
    want = dict(obs=np.zeros((B, A, v, v, 3), np.uint8), dir=np.zeros((B, A), np.uint8), reward=np.zeros((B, A)),
                terminated=np.zeros((B, A), np.uint8), truncated=np.zeros(B, np.uint8))
    raised = []
    for b in range(B):
        s = slice(b, b + 1)
        try:
            out = ob.step_batch(sd, st["grid"][s], st["agents"][s], st["rng"][s], st["step_count"][s], act[s], aux[s])
        except ValueError:
            raised.append(b)
            continue
        for k, o in zip(OUTS, out):
            want[k][b] = o[0]
    # (an agent that an ends-all event of an EARLIER agent terminated is skipped before its action is looked at, base.py:408-409:
    # such an env raises nothing, in the reference and here)
    assert set(raised) <= {b for b in range(B) if b % 4} and all(any(b % 4 == k for b in raised) for k in (1, 2, 3))
    env = fx.env(B)
    outs = env.step(torch.from_numpy(act).to(DEV))
    env.join()
    err = [int(x) for x in env.err.cpu()]
    assert err == [len(raised), raised[0]], (err, len(raised), raised[0])
    clean = np.array([b for b in range(B) if b not in raised])
    _compare(env, outs, dict(want, **st), clean, f"{name} unknown action")
    _compare(env, outs, dict(grid=z["grid"][0], agents=z["agents"][0], obs=z["obs"][0]), np.arange(0, B, 4),
             f"{name} unknown action (reference)")
    with pytest.raises(ValueError, match="Unknown action"):
        env.check_errors()
