"""BatchedMultiGridEnv.reset(seed, mask) on the device: mgx_reset_generate_select / mgx_reset_select against the oracle-backed env of
tests/test_reset_select.py and the recorded bytes of the reference (resets_*.npz, seeded/seeded_resets.npz).  Every comparison is
torch.equal: cells, agents, aux, rng, gen_state, step_count, episode, was_reset and the observation reset() returns.

Batches of 1, 63 and 130 envs (two full wavefronts and a two-lane tail) under every mask that picks a different path of the scan --
nobody, everybody, None, lane 0, lane 63, the tail's last lane, every other env, a whole wavefront left out -- with a running env
among the selected and a finished env among the others; the pool form at 300 envs (a full workgroup and a 44-env wavefront) in every
copy unit; the staging slots of a staged generator across a reset; reset_done() against reset(mask=is_done()) -- one body behind two
triggers -- in both forms; and the whole file again on the bounds-checked build."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib
from tests import util
from tests.test_reference_resets import check_state, load
from tests.test_reference_resets_gpu import spread, stepping_env
from tests.test_reset_select import (SEEDED_TAGS, STATE, Seeded, SelectOracle, alternating, check_pool, check_seeded, live_env,
                                     pool_env, snapshot, sub_env)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: the smallest recorded size of each generator kind
GEN_FIXTURES = ("resets_empty_fixed_5_a3", "resets_empty_random_6_a3", "resets_bup_rs5_a2", "resets_rbd_5_a2",
                "resets_lh_2rooms_rs5_k33_a2", "resets_playground_1x1_rs7_a1")


def masks(N):
    """{name: bool[N] or None}: every path of the one-lane-per-env scan at this batch"""
    b = torch.arange(N)
    out = {"none": torch.zeros(N, dtype=torch.bool), "all": torch.ones(N, dtype=torch.bool), "None": None, "lane0": b == 0,
           "tail_last": b == N - 1, "alternating": b % 2 == 0}
    if N > 63:
        out["lane63"] = b == 63
    if N > 64:
        out["wave0_none_wave1_all"] = (b >= 64) & (b < 128)
    return out


def restore(env, snap):
    for k, v in snap.items():
        (env._gen["gen_state"] if k == "gen_state" else getattr(env, k)).copy_(v)


def same_as(dev_env, cpu_env, obs_d, obs_c, ctx):
    got, want = snapshot(dev_env), snapshot(cpu_env)
    for k in want:
        assert torch.equal(got[k], want[k]), f"{ctx}: {k} differs from the oracle-backed env's"
    assert torch.equal(dev_env.was_reset.cpu(), cpu_env.was_reset), f"{ctx}: was_reset"
    assert torch.equal(obs_d[0].cpu(), obs_c[0]) and torch.equal(obs_d[1].cpu(), obs_c[1]), f"{ctx}: the observation reset() returns"


def first_unselected(mask, N):
    if mask is None:
        return ()
    rest = (~mask).nonzero().flatten()
    return (int(rest[0]),) if len(rest) else ()


@pytest.mark.parametrize("name", GEN_FIXTURES)
def test_generated_restarts_of_selected_envs(name):
    z, d, spec, gen = load(name)
    E = len(z["lay_before"])
    for N in (1, 63, 130):
        idx = spread(E, N)
        dev_env = live_env(z, spec, gen, idx, DEV)
        cpu_env = live_env(z, spec, gen, idx, "cpu", backend=SelectOracle(spec))
        base = snapshot(cpu_env)
        for mname, mask in masks(N).items():
            for seed in (None, 5):
                ctx = f"{name} B={N} mask={mname} seed={seed}"
                for e in (dev_env, cpu_env):
                    restore(e, base)
                    for b in first_unselected(mask, N):                 # a finished env that is not selected (everybody else runs)
                        e.step_count[b] = spec.max_steps
                    e.was_reset.fill_(7)
                before = snapshot(dev_env)
                obs_d = dev_env.reset(seed=seed, mask=None if mask is None else mask.to(DEV))
                obs_c = cpu_env.reset(seed=seed, mask=mask)
                same_as(dev_env, cpu_env, obs_d, obs_c, ctx)
                sel = np.arange(N) if mask is None else mask.nonzero().flatten().numpy()
                keep = torch.ones(N, dtype=torch.bool)
                keep[sel] = False
                after = snapshot(dev_env)
                for k in after:
                    assert torch.equal(after[k][keep], before[k][keep]), f"{ctx}: {k} of an env that was not selected changed"
                if seed is None and len(sel):                            # the reference's recorded bytes
                    check_state(sub_env(dev_env, sel), z, gen, idx[sel], ctx)
                    assert torch.equal(obs_d[0][torch.as_tensor(sel, device=DEV)].cpu(), torch.from_numpy(z["obs0"][idx[sel]])), ctx
                elif len(sel):
                    check_seeded(dev_env, z, gen, idx, 5, sel[:3].tolist() + sel[-2:].tolist(), ctx)
        dev_env.check_errors()


@pytest.mark.parametrize("tag", SEEDED_TAGS)
def test_seeded_generation_reproduces_the_references_seeded_resets(tag):
    """reset(seed=s) of global env 0 == the reference's recorded reset(seed=s) -- BlockedUnlockPickup's door row and Playground's door
    positions come from the NEW stream, a pending half of the old one is dropped --; other global indices == the oracle-backed env."""
    z = Seeded(tag)
    for n, seed in enumerate(z["seed"].tolist()):
        env = live_env(z, z.spec, z.gen, np.array([n]), DEV)
        obs, _ = env.reset(seed=seed)
        check_state(env, z, z.gen, np.array([n]), f"{tag} seed {seed}")
        assert torch.equal(obs.cpu(), torch.from_numpy(z["obs0"][n:n + 1])), f"{tag} seed {seed}: first observation"
    N = 130
    idx = spread(len(z["seed"]), N)
    dev_env = live_env(z, z.spec, z.gen, idx, DEV, first_env=3)
    cpu_env = live_env(z, z.spec, z.gen, idx, "cpu", backend=SelectOracle(z.spec), first_env=3)
    mask = alternating(N)
    same_as(dev_env, cpu_env, dev_env.reset(seed=11, mask=mask.to(DEV)), cpu_env.reset(seed=11, mask=mask), f"{tag} first_env=3")
    check_seeded(dev_env, z, z.gen, idx, 11, [0, 2, 64, 128], f"{tag} first_env=3")
    dev_env.check_errors()


def test_a_seeded_restart_draws_the_door_row_from_the_new_stream():
    """(that the comparison above can tell: over the recorded events, the seeded and the unseeded restart of the same env differ)"""
    z = Seeded("bup_rs5_a2")
    differ = 0
    for n, seed in enumerate(z["seed"].tolist()):
        a, b = live_env(z, z.spec, z.gen, np.array([n]), DEV), live_env(z, z.spec, z.gen, np.array([n]), DEV)
        a.reset(seed=seed); b.reset()
        assert torch.equal(a._gen["gen_state"][:, 2:4], b._gen["gen_state"][:, 2:4]), "the placement stream is not re-seeded"
        assert not torch.equal(a.rng, b.rng)
        differ += int(not torch.equal(a.cells, b.cells))
    assert differ >= 1


# ---- staging slots across a reset ------------------------------------------------------------------------------------------------------

OUTPUTS = ("obs", "dir", "reward", "terminated", "truncated", "was_reset")


def staging_run(mode, graph=False):
    """resets_con_bup_rs6_a3: step to one step before every env's truncation (slots and snapshots exist), reset(seed=7) every other
    env, step past the other envs' truncation and on to the selected envs' own.  Returns the per-step records (the last one only for
    the graph form: the steps after the reset are one captured graph, replayed once)."""
    name = "resets_con_bup_rs6_a3"
    z, d, spec, gen = load(name)
    E = len(z["lay_before"])
    N = 8 * E + 5
    idx = spread(E, N)
    lead = 4
    pre = lead + 2                                           # steps before the reset: one short of the truncation
    env = stepping_env(z, spec, gen, idx, pre + 1, mode, None if mode is False else 2 if mode in ("candidates", "in_launch") else lead)
    T = env.spec.max_steps + 1
    A = spec.num_agents
    # left / right / forward / absent: the agents move about, nobody picks the target up -- every episode ends by truncation
    acts = torch.from_numpy(np.random.default_rng(100).integers(-1, 3, size=(pre + T, N, A)).astype(np.int8)).to(DEV)
    for t in range(pre):
        env.step(acts[t], auto_reset=True)
    assert int(env.step_count[0]) == env.spec.max_steps - 1 and not bool(env.was_reset.any())
    st = env._gen.get("stage")
    if st is not None:
        held = (st["tag"][:, :st["candidates"]] == env.episode[:, None]).all(dim=1) if st.get("candidates") else (st["tag"][:, 0] >= 0) | (st["tag"][:, 3] != 0)
        assert int(held.sum()) == N, f"{mode}: the slots / snapshots the reset must invalidate are not there"
    rec = lambda: {**snapshot(env), **{k: getattr(env, k).cpu().clone() for k in OUTPUTS}}
    mask = alternating(N, DEV)
    if graph:
        g = env.capture_steps(acts[pre:], auto_reset=True)
        env.reset(seed=7, mask=mask)
        g.replay()
        torch.cuda.synchronize()
        env.check_errors()
        return [rec()]
    env.reset(seed=7, mask=mask)
    out = [rec()]
    for t in range(pre, pre + T):
        env.step(acts[t], auto_reset=True)
        out.append(rec())
    env.check_errors()
    sel = mask.cpu()
    # the others truncated with the first step after the reset, the selected envs with the max_steps-th
    assert torch.equal(out[1]["truncated"].bool(), ~sel) and bool(out[env.spec.max_steps]["truncated"][sel].all())
    return out


@pytest.fixture(scope="module")
def unstaged():
    return staging_run(False)


@pytest.mark.parametrize("mode", ["candidates", "between", "in_launch", False], ids=lambda m: str(m))
def test_staging_slots_stay_correct_across_a_reset(mode, unstaged):
    """The slots are a cache keyed by the episode counter: a restart bumps it, so what was staged for the abandoned episode is never
    adopted -- states and outputs equal the unstaged run's at every step, eagerly and through a captured graph replayed after the
    reset."""
    if mode is not False:
        got = staging_run(mode)
        assert len(got) == len(unstaged)
        for t, (g, w) in enumerate(zip(got, unstaged)):
            for k in w:
                assert torch.equal(g[k], w[k]), f"{mode}: {k} differs from the unstaged run's {t} steps after the reset"
    last = staging_run(mode, graph=True)[0]
    for k in unstaged[-1]:
        assert torch.equal(last[k], unstaged[-1][k]), f"{mode} graph: {k} differs from the unstaged run's after the last step"


# ---- the pool form ---------------------------------------------------------------------------------------------------------------------

#: layout bytes -> the copy unit reset_copy_unit picks (mgx_aux_geom.h); the last two reach the 8- and 2-byte instantiations
POOL_SPECS = {"empty8_a1_c2_128B_uint4": EnvSpec(8, 8, 1, 7, max_steps=20),
              "9x7_a3_c3_189B_bytes": EnvSpec(9, 7, 3, 5, max_steps=20, cell_bytes=3),
              "64x64_a2_c1_4096B_uint4": EnvSpec(64, 64, 2, 7, max_steps=20, cell_bytes=1),
              "bup_11x6_a2_c2_132B_uint32": EnvSpec(11, 6, 2, 7, max_steps=20, joint_reward=True, env_kind="blockedunlockpickup"),
              "6x6_a2_c2_72B_uint64": EnvSpec(6, 6, 2, 5, max_steps=20),
              "5x5_a1_c2_50B_uint16": EnvSpec(5, 5, 1, 3, max_steps=20)}


@pytest.mark.parametrize("name", list(POOL_SPECS))
def test_pool_restarts_of_selected_envs(name):
    spec, B = POOL_SPECS[name], 300
    dev_env, pool = pool_env(spec, B, DEV, first_env=4)
    cpu_env, _ = pool_env(spec, B, "cpu", first_env=4, backend=SelectOracle(spec))
    base = snapshot(cpu_env)
    for mname, mask in masks(B).items():
        for seed in (None, 6):
            ctx = f"{name} mask={mname} seed={seed}"
            for e in (dev_env, cpu_env):
                restore(e, base)
                for b in first_unselected(mask, B):
                    e.step_count[b] = spec.max_steps
                e.was_reset.fill_(7)
            before = snapshot(dev_env)
            obs_d = dev_env.reset(seed=seed, mask=None if mask is None else mask.to(DEV))
            obs_c = cpu_env.reset(seed=seed, mask=mask)
            same_as(dev_env, cpu_env, obs_d, obs_c, ctx)
            check_pool(dev_env, pool, before, mask, seed, ctx)
    dev_env.check_errors()


def test_first_episode_from_reset_alone():
    """Nothing loaded: reset(seed) of the whole batch IS the initial state -- the README's quick start."""
    z = Seeded("bup_rs5_a2")
    envs = []
    for dev, kw in ((DEV, {}), ("cpu", dict(backend=SelectOracle(z.spec)))):
        env = BatchedMultiGridEnv(z.spec, 130, dev, **kw)
        env.set_layout_generator("blockedunlockpickup", layout_seed=2, room_size=z.gen["room_size"])
        envs.append((env, env.reset(seed=0)))
    same_as(envs[0][0], envs[1][0], envs[0][1], envs[1][1], "first episode")
    envs[0][0].step(torch.zeros((130, z.spec.num_agents), dtype=torch.int8, device=DEV), auto_reset=True)
    envs[0][0].check_errors()


# ---- one body, two triggers ---------------------------------------------------------------------------------------------------------------

def finish(env, envs):
    """of `envs`: b % 3 == 0 ends by step_count = max_steps, b % 3 == 1 by every agent's terminated byte, b % 3 == 2 runs on"""
    b = torch.as_tensor(envs, device=env.cells.device)
    env.step_count[b[b % 3 == 0]] = env.spec.max_steps
    env.agents[b[b % 3 == 1], :, 4] = 1


def pairs_of_envs(form):
    """(name, two device envs in the same state with the same finished envs) -- every pool spec at 300 envs: the wavefront of envs
    128..191 has nobody finished; every generator kind at 130 envs: nobody in wavefront 0, wavefront 1 mixed, env 129 of the two-lane
    tail finished"""
    if form == "pool":
        for name, spec in POOL_SPECS.items():
            envs = [pool_env(spec, 300, DEV, first_env=4)[0] for _ in range(2)]
            for e in envs:
                finish(e, [b for b in range(300) if not 128 <= b < 192])
            yield name, envs
    else:
        for name in GEN_FIXTURES:
            z, d, spec, gen = load(name)
            idx = spread(len(z["lay_before"]), 130)
            envs = [live_env(z, spec, gen, idx, DEV) for _ in range(2)]
            for e in envs:
                finish(e, range(64, 130))
            yield name, envs


@pytest.mark.parametrize("form", ["pool", "generator"])
def test_done_restart_equals_select_of_is_done(form):
    """reset_done() and reset(mask = is_done()) run the same body behind two triggers: every byte of the state they leave is the same."""
    for name, (by_done, by_select) in pairs_of_envs(form):
        done = by_done.is_done()
        assert torch.equal(done, by_select.is_done())
        lo = 128 if form == "pool" else 0
        assert not bool(done[lo:lo + 64].any()) and bool(done[64:128].any()) and not bool(done[64:128].all()), name
        assert bool(done[-1]) == (form == "generator") and 0 < int(done.sum()) < len(done)
        for e in (by_done, by_select):
            e.was_reset.fill_(7)
        by_done.reset_done()
        by_select.reset(mask=done.clone())
        a, b = snapshot(by_done), snapshot(by_select)
        assert set(a) == set(b) and (form == "pool" or "gen_state" in a)
        for k in a:
            assert torch.equal(a[k], b[k]), f"{name}: {k} after reset_done() differs from reset(mask=is_done())"
        assert torch.equal(by_done.was_reset, by_select.was_reset) and torch.equal(by_done.was_reset.bool(), done), name
        assert not bool(by_done.is_done().any()), name
        by_done.check_errors(); by_select.check_errors()


# ------------------------------------------------------------------------------------------------------------ bounds-checked build

def test_bounds_checked_build_counts_no_violation():
    """Only meaningful inside the bounds-checked run below (MGX_LIBMGX = libmgx_chk.so), where it is collected LAST: after every test
    of this file, no LDS access left its wavefront's slice.  In the ordinary run it checks nothing and says so by returning at once;
    the outer test below fails unless the line this test prints in the inner run is there."""
    from multigrid_amd import build
    if os.environ.get("MGX_LIBMGX") != build.LIB_CHK:
        return
    v = (ctypes.c_int32 * 2)()
    assert _lib.lib().mgx_debug_bounds_violations(v) == 0
    assert v[0] == 0, f"{v[0]} LDS accesses outside their wavefront's slice (last site {v[1]})"
    print(f"bounds check: {v[0]} LDS accesses outside their wavefront's slice")


def test_the_whole_file_on_the_bounds_checked_build():
    from multigrid_amd import build
    if os.environ.get("MGX_LIBMGX") == build.LIB_CHK:
        return                                        # (this is the inner run)
    assert os.path.exists(build.LIB_CHK), "libmgx_chk.so is missing: __graft_entry__.build() makes it"
    # (-x: the inner run ends at its first failure -- nothing more is started on a device a test may have faulted)
    cmd = [sys.executable, "-m", "pytest", "-q", "-s", "-x", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__),
           "-k", "not the_whole_file"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, MGX_LIBMGX=build.LIB_CHK))
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "bounds check: 0 LDS accesses" in out.stdout, out.stdout[-1000:]
