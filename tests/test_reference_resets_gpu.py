"""Device-side episode generation against the REFERENCE's own resets (tests/golden/resets_*.npz; the CPU side and the helpers:
tests/test_reference_resets.py).  One env of a batch is one recorded reset event: finished (or about to be), with the recorded
pre-states of the placement generator and of env.np_random written into `gen_state` / `rng`.  The events are replicated along the
batch, shifted by one env per replica so that an event meets every lane of a group of eight, in batches that are no multiple of 64.
Every comparison is torch.equal against recorded bytes: cells (unpacked), agents, aux, rng, gen_state, step_count, episode, was_reset.

Families: reset_done() (mgx_reset_generate); step(auto_reset=True) unstaged, plain and one-hot (the tail of mgx_step_generate); the
staging modes "candidates" / "between" / "side" / "in_launch" eagerly, as a captured graph and as rollout() -- the candidates
kernel places with groups of eight lanes (mgx_layout_gen.h place_group), so the constructed re-sampling states reach its serial
fallback and its ignored later tries on recorded truth; and the whole file again on the bounds-checked build, whose faked re-sample
claims send about every tenth place_obj call through the fallback."""
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multigrid_amd import _lib
from tests import util
from multigrid_amd import BatchedMultiGridEnv
from oracle import binding as ob
from tests.test_reference_resets import chain_aux, check_state, inject, layouts_py, load, load_chain, make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MULT = 0x2360ED051FC65DA44385DF649FCCF645
_INV = pow(_MULT, -1, 1 << 128)
DONE = 6                                       # Action.done: changes nothing


def spread(E, N):
    """env b of N <- event (b + b // E) % E: every replica of the E events is shifted by one lane"""
    b = np.arange(N)
    return (b + b // E) % E


def batch_sizes(E):
    return (E, 8 * E + 5, 64 * 3 + 7 * E + 1)


def rewound(words5, words):
    """PCG64 words as they were `words` 64-bit draws earlier (np_random before the steps' action-order draws, base.py:396-399)"""
    out = np.array(words5[:, :4], dtype=np.uint64)
    for r, w in enumerate(words5):
        s, inc = int(w[0]) | (int(w[1]) << 64), int(w[2]) | (int(w[3]) << 64)
        for _ in range(words):
            s = ((s - inc) * _INV) & ((1 << 128) - 1)
        out[r, 0], out[r, 1] = s & ((1 << 64) - 1), s >> 64
    return out


def stepping_env(z, spec, gen, idx, steps, staged, lead=None):
    """env b = event idx[b], `steps` steps before its truncation: np_random stands `steps` action-order draws before the recorded
    pre-state, the placement generator at it"""
    sp = dataclasses.replace(spec, max_steps=steps + 9)
    env = make_env(z, sp, gen, idx, DEV)
    if staged is not False:
        env.set_layout_generator(gen["kind"], layout_seed=1, room_size=gen["room_size"], start=tuple(gen["start"]),
                                 max_hallway_keys=gen["max_hallway_keys"], max_keys_per_room=gen["max_keys_per_room"], staged=staged, lead=lead)
        inject(env, z, idx)
    per_step = spec.num_agents if spec.num_agents > 1 else 0
    env.rng.copy_(torch.from_numpy(rewound(z["npr_before"][idx], steps * per_step).view(np.int64)))
    env.step_count.fill_(sp.max_steps - steps)
    return env


@pytest.mark.parametrize("name", util.RESETS_IDS)
def test_reset_generate_reproduces_every_recorded_reset(name):
    z, d, spec, gen = load(name)
    E = len(z["lay_before"])
    for N in batch_sizes(E):
        idx = spread(E, N)
        env = make_env(z, spec, gen, idx, DEV)
        assert int(env.reset_done().sum()) == N
        check_state(env, z, gen, idx, f"{name} B={N}")
        env.gen_obs()
        assert torch.equal(env.obs.cpu(), torch.from_numpy(z["obs0"][idx])), f"{name} B={N}: first observation"
        env.check_errors()


@pytest.mark.parametrize("one_hot", [False, True], ids=["plain", "one_hot"])
@pytest.mark.parametrize("name", util.RESETS_IDS)
def test_step_generate_tail_reproduces_every_recorded_reset(name, one_hot):
    z, d, spec, gen = load(name)
    E = len(z["lay_before"])
    N = 8 * E + 5
    idx = spread(E, N)
    env = stepping_env(z, spec, gen, idx, 1, False)
    act = torch.full((N, spec.num_agents), DONE, dtype=torch.int8, device=DEV)
    out = env.step(act, auto_reset=True, one_hot=one_hot)
    # (the step returns the ENDED episode's last observation -- here of a made-up state --, not the new episode's: its recorded
    # outputs are the flags; the chains below compare every output of resetting steps with the reference's)
    assert bool(out[4].all()), "every env truncates with this step"
    assert not bool(out[3].any()) and not bool(out[2].any()), "nobody terminated, nobody was paid"
    check_state(env, z, gen, idx, f"{name} one_hot={one_hot}")
    obs0 = z["obs0"][idx]
    got, _ = env.gen_obs(one_hot=one_hot)                # the new episode's first observation, through the same output path
    assert torch.equal(got.cpu(), torch.from_numpy(ob.one_hot(obs0) if one_hot else obs0)), f"{name}: first observation"
    env.check_errors()


#: (fixture, mode): the constructed re-sampling states and the exactly full rooms, under every staging mode their generator has
STAGED = [(n, m) for n, modes in (
    ("resets_con_empty_random_6_a3", ("candidates", "between", "in_launch")),
    ("resets_con_bup_rs6_a3", ("candidates", "between", "side", "in_launch")),
    ("resets_con_bup_rs7_a2", ("between", "side")),
    ("resets_con_rbd_6_a3", ("candidates", "side")),
    ("resets_con_lh_6rooms_rs5_k23_a3", ("candidates", "between")),
    ("resets_con_playground_2x3_rs6_a2", ("between", "in_launch")),
    ("resets_bup_rs4_a2_full", ("candidates",)), ("resets_bup_rs5_a7_full", ("candidates",)),
    ("resets_lh_2rooms_rs4_k11_a3_full", ("candidates",)), ("resets_rbd_4_a4_full", ("candidates",)),
    ("resets_empty_random_5_a8_full", ("candidates",)), ("resets_lh_16rooms_rs7_k33_a4", ("candidates", "between")),
    ("resets_bup_rs9_a2", ("between",)), ("resets_playground_4x4_rs6_a3", ("between",))) for m in modes]


@pytest.mark.parametrize("name,mode", STAGED, ids=[f"{n}-{m}" for n, m in STAGED])
def test_staged_generation_reproduces_recorded_resets(name, mode):
    """The slots are filled by generator launches while the episode runs and adopted by the step that truncates it: the adopted
    start must be the reference's -- eagerly, as a captured graph, and as rollout().  The adoptions must actually happen."""
    z, d, spec, gen = load(name)
    E = len(z["lay_before"])
    N = 8 * E + 5
    idx = spread(E, N)
    lead = 2 if mode in ("candidates", "in_launch") else 4
    steps = lead + 3
    acts = torch.full((steps, N, spec.num_agents), DONE, dtype=torch.int8, device=DEV)

    def served(env, ready=False):
        """envs whose slots hold something; ready: every candidate of the env's CURRENT episode's successor is there"""
        st = env._gen["stage"]
        if ready:
            return int((st["tag"][:, :st["candidates"]] == env.episode[:, None]).all(dim=1).sum())
        return int((st["tag"][:, 0] >= 0).sum())

    env = stepping_env(z, spec, gen, idx, steps, mode, lead)
    assert env._gen["stage"]["lead"] == lead and bool(env._gen["stage"].get("candidates")) == (mode == "candidates")
    for t in range(steps):
        if t == steps - 1 and mode == "candidates":
            assert served(env, True) == N, "a candidate was not ready before the truncating step"
        out = env.step(acts[t], auto_reset=True)
        assert bool(out[4].all()) == (t == steps - 1)
    torch.cuda.synchronize()
    check_state(env, z, gen, idx, f"{name} {mode} eager")
    assert served(env) == N, served(env)
    env.check_errors()
    env = stepping_env(z, spec, gen, idx, steps, mode, lead)
    graph = env.capture_steps(acts, auto_reset=True)
    graph.replay()
    torch.cuda.synchronize()
    check_state(env, z, gen, idx, f"{name} {mode} graph")
    assert served(env) == N, served(env)
    env.check_errors()
    if mode in ("between", "candidates"):
        # rollout(): every step's obs slice must be 16-byte aligned (include/mgx.h) -- a batch of 16 * odd envs: no multiple of 64
        N = 16 * (((8 * E + 5) // 16) | 1)
        assert N % 64 and (N * spec.num_agents * spec.view_size ** 2 * 3) % 16 == 0
        idx = spread(E, N)
        acts = torch.full((steps, N, spec.num_agents), DONE, dtype=torch.int8, device=DEV)
        env = stepping_env(z, spec, gen, idx, steps, mode, lead)
        out = env.rollout(acts, auto_reset=True)
        assert bool(out["was_reset"][-1].all()) and not bool(out["was_reset"][:-1].any())
        env.was_reset.copy_(out["was_reset"][-1])       # (rollout() hands was_reset[T,B] back; check_state reads the env's)
        check_state(env, z, gen, idx, f"{name} {mode} rollout")
        assert served(env) == N, served(env)
        env.check_errors()


def test_sub_shard_chains_reproduce_recorded_resets():
    """capture_steps(sub_shards=2) and split(): every shard generates its own slice of the batch."""
    name = "resets_con_bup_rs6_a3"
    z, d, spec, gen = load(name)
    E = len(z["lay_before"])
    N = 512 + 8 * E
    idx = spread(E, N)
    steps = 5
    acts = torch.full((steps, N, spec.num_agents), DONE, dtype=torch.int8, device=DEV)
    env = stepping_env(z, spec, gen, idx, steps, "candidates", 2)
    graph = env.capture_steps(acts, auto_reset=True, sub_shards=2)
    graph.replay()
    torch.cuda.synchronize()
    check_state(env, z, gen, idx, f"{name} sub-shard graph")
    env.check_errors()
    env = stepping_env(z, spec, gen, idx, 1, False)
    lo = 0
    for part in env.split(2):
        part.step(acts[0, lo:lo + part.batch], auto_reset=True)
        lo += part.batch
    torch.cuda.synchronize()
    assert lo == N
    check_state(env, z, gen, idx, f"{name} split()")
    env.check_errors()


# ---- chained episodes: early ends and truncations, every step's outputs (tests/golden/resets_chain_*.npz) --------------------------

class Chain:
    def __init__(self, name):
        self.name = name
        self.z, self.d, self.spec, self.gen = load_chain(name)
        z = self.z
        self.T, self.A = len(z["actions"]), self.spec.num_agents
        self.edits = {int(t): row for t, row in zip(z["edit_step"], z["edit_row"])}
        self.cuts = sorted(set([0, self.T] + list(self.edits)))                 # segments without an edit inside

    def env(self, N, staged, lead=None):
        z, gen = self.z, self.gen
        env = BatchedMultiGridEnv(self.spec, N, DEV)
        rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (N,) + a.shape))
        env.load_state(rep(z["grid0"][0]), rep(z["agents0"][0]), rep(z["npr_after"][0, :4]),
                       rep(chain_aux(z, gen, 0)) if self.spec.env_kind != "empty" else None)
        env.set_layout_generator(gen["kind"], layout_seed=1, room_size=gen["room_size"], staged=staged, lead=lead)
        gs = np.zeros((N, 6), np.uint64)
        gs[:, :5] = z["lay_after"][0]; gs[:, 5] = z["npr_after"][0, 4]
        env._gen["gen_state"].copy_(torch.from_numpy(gs.view(np.int64)))
        return env

    def actions(self, N):
        return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(self.z["actions"][:, None, :], (self.T, N, self.A)))).to(DEV)

    def edit(self, env, t):
        if t in self.edits:
            env.agents[:, 0, :] = torch.from_numpy(self.edits[t].copy()).to(DEV)

    def same(self, got, want, ctx, what):
        got = got.cpu()
        want = torch.from_numpy(np.ascontiguousarray(want).reshape(-1))
        if got.dtype != want.dtype:
            want = want.view(got.dtype)
        assert torch.equal(got, want.reshape(got.shape[1:]).unsqueeze(0).expand_as(got)), f"{self.name} {ctx}: {what} differs from the reference's"

    def check_outputs(self, outs, t, ctx):
        z = self.z
        for got, key in zip(outs, ("obs", "dir", "reward", "terminated", "truncated")):
            self.same(got, z[key][t], ctx, key)

    def check_state(self, env, t, ctx):
        z, r = self.z, int(self.z["reset_of"][t])
        gs = env._gen["gen_state"]
        if r >= 0:
            self.same(env.grid, z["grid0"][r], ctx, "grid after the reset"); self.same(env.agents, z["agents0"][r], ctx, "agents after the reset")
            self.same(env.rng, z["npr_after"][r, :4].view(np.int64), ctx, "rng after the reset")
            self.same(gs[:, :5], z["lay_after"][r].view(np.int64), ctx, "gen_state[:, :5]")
            self.same(gs[:, 5], z["npr_after"][r, 4:5].view(np.int64)[0], ctx, "gen_state[:, 5]")
            if self.spec.env_kind != "empty":
                self.same(env.aux, chain_aux(z, self.gen, r), ctx, "aux")
        else:
            self.same(env.grid, z["grid"][t], ctx, "grid"); self.same(env.agents, z["agents"][t], ctx, "agents")
            self.same(env.rng, z["npr"][t, :4].view(np.int64), ctx, "rng")
        steps_in = t - int(np.nonzero(z["done"][:t + 1])[0].max()) if z["done"][:t + 1].any() else t + 1
        self.same(env.step_count, np.int32(steps_in), ctx, "step_count")
        self.same(env.episode, np.int32(int(z["done"][:t + 1].sum())), ctx, "episode")


CHAIN_MODES = [(n, m) for n in util.RESETS_CHAIN_IDS for m in (False, "candidates", "between", "side", "in_launch")
               if not (m == "candidates" and "rs8" in n)]              # (6 door rows: no candidates protocol, mgx_layout_gen.h)


@pytest.mark.parametrize("name,mode", CHAIN_MODES, ids=[f"{n}-{m or 'unstaged'}" for n, m in CHAIN_MODES])
def test_chain_replays_on_the_device(name, mode):
    """step(auto_reset=True) over a recorded chain -- eagerly (every step's outputs, state and was_reset), as rollout() segments and as
    captured graphs (cut where the recording edits agent 0) -- unstaged, one-hot, and under every staging mode, whose slots must be
    used: an early end adopts its candidate like a truncation does."""
    ch = Chain(name)
    z, T = ch.z, ch.T
    N = 16 * 13                                             # 208 envs: 16-byte aligned output slices, no multiple of 64
    acts = ch.actions(N)
    lead = None if mode is False else 2 if mode in ("candidates", "in_launch") else 4
    env = ch.env(N, mode, lead)
    ready_at_end, ends = 0, 0
    for t in range(T):
        ch.edit(env, t)
        if mode == "candidates" and z["done"][t]:
            st = env._gen["stage"]
            ends += 1
            ready_at_end += int(bool((st["tag"][:, :st["candidates"]] == env.episode[:, None]).all()))
        outs = env.step(acts[t], auto_reset=True)
        ch.check_outputs(outs, t, f"{mode} step {t}")
        ch.same(env.was_reset, z["done"][t], f"{mode} step {t}", "was_reset")
        ch.check_state(env, t, f"{mode} step {t}")
    env.check_errors()
    if mode == "candidates":
        early = int((z["done"].astype(bool) & ~z["truncated"].astype(bool)).sum())
        print(f"{name}: candidates ready at {ready_at_end} of {ends} episode ends ({early} early)")
        assert ready_at_end == ends, (ready_at_end, ends)    # a generator launch follows every step (lead 2): always there
    elif mode:
        assert int((env._gen["stage"]["tag"][:, 0] >= 0).sum()) == N
    if mode is False:                                        # the one-hot form of the same launches
        env = ch.env(N, False)
        for t in range(T):
            ch.edit(env, t)
            outs = env.step(acts[t], auto_reset=True, one_hot=True)
            ch.same(outs[0], ob.one_hot(z["obs"][t]), f"one-hot step {t}", "one-hot obs")
            ch.check_state(env, t, f"one-hot step {t}")
    if mode in (False, "candidates", "between"):
        env = ch.env(N, mode, lead)
        for a, b in zip(ch.cuts[:-1], ch.cuts[1:]):
            ch.edit(env, a)
            out = env.rollout(acts[a:b], auto_reset=True)
            for t in range(a, b):
                ch.check_outputs([out[k][t - a] for k in ("obs", "dir", "reward", "terminated", "truncated")], t, f"{mode} rollout step {t}")
                ch.same(out["was_reset"][t - a], z["done"][t], f"{mode} rollout step {t}", "was_reset")
            ch.check_state(env, b - 1, f"{mode} rollout step {b - 1}")
        env.check_errors()
    env = ch.env(N, mode, lead)
    for a, b in zip(ch.cuts[:-1], ch.cuts[1:]):
        ch.edit(env, a)
        graph = env.capture_steps(acts[a:b], auto_reset=True)
        graph.replay()
        torch.cuda.synchronize()
        ch.check_outputs([env.obs, env.dir, env.reward, env.terminated, env.truncated], b - 1, f"{mode} graph step {b - 1}")
        ch.check_state(env, b - 1, f"{mode} graph step {b - 1}")
    env.check_errors()


def test_chain_on_sub_shards():
    """split(): the shards of one batch step the chain on their own; capture_steps(sub_shards=2): two chains of launches in one graph."""
    ch = Chain("resets_chain_bup_rs6_a2")
    N = 512 + 48
    acts = ch.actions(N)
    env = ch.env(N, "candidates", 2)
    for a, b in zip(ch.cuts[:-1], ch.cuts[1:]):
        ch.edit(env, a)
        graph = env.capture_steps(acts[a:b], auto_reset=True, sub_shards=2)
        graph.replay()
        torch.cuda.synchronize()
        ch.check_state(env, b - 1, f"sub-shard graph step {b - 1}")
    env.check_errors()
    env = ch.env(N, False)
    parts = env.split(2)
    for t in range(ch.T):
        ch.edit(env, t)
        lo = 0
        for part in parts:
            outs = part.step(acts[t, lo:lo + part.batch], auto_reset=True)
            ch.check_outputs(outs, t, f"split() step {t}")
            lo += part.batch
        torch.cuda.synchronize()
        ch.check_state(env, t, f"split() step {t}")
    env.check_errors()


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
    cmd = [sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__),
           "-k", "not the_whole_file"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=850, cwd=ROOT, env=dict(os.environ, MGX_LIBMGX=build.LIB_CHK))
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "bounds check: 0 LDS accesses" in out.stdout, out.stdout[-1000:]
