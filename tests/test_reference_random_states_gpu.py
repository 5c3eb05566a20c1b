"""Every step-kernel family against the REFERENCE's own bytes on random states (tests/golden/randstate_*.npz, written by
oracle/gen_golden.py: record_random_states -- batches of tests.util.random_state envs loaded into ini/multigrid and stepped there).

The other GPU parity tests compare the kernels with the C oracle; this file compares them with what the reference recorded, so a
misreading of multigrid/base.py:378-476 or utils/obs.py shared by the oracle and a kernel fails here.  A fixture of B_f envs is
replicated along the batch: env n of a launch holds fixture env n % B_f (same state, same actions), so one vectorised compare on the
device checks every replica, and the replicas start each wavefront's observation bytes at every residue the dword-staged P4/P5 sees.
Checked every step: obs, dir, reward (bytes), terminated, truncated; and the grid, agents, generator words and step count.

Families: latency (one replica and a ragged batch), throughput (> 2048 wavefronts), the shape-specialised instantiations and
specialise() (hipRTC), compact and byte-grid cells, the fused one-hot output, the rollout, the resident rollout shapes (7 / 8 / 9), the
persistent launch (plain and resident), sub-shard chains (captured and eager) -- and the whole file again on the bounds-checked
build.  Also: the reward expression of base.py:602 at every step count of a set of max_steps, in the plain, one-hot and auto-reset
launches."""
import contextlib
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib
from oracle import binding as ob
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = dict(zip(util.RANDSTATE_IDS, util.RANDSTATE_GOLDEN))
C24 = "randstate_16x16_a4_v7"              # the C2 / C4 shape
C5 = "randstate_64x64_a16_v9"              # the C5 shape (no filled boxes: compact-cell eligible)
BUP = "randstate_bup_11x6_a2_v7"           # the C3 shape
BOXES = "randstate_10x9_a3_v7_boxes"       # filled boxes: refused by compact cells


class Fixture:
    def __init__(self, name, path=None):
        self.name = name
        self.z, self.d, self.spec = util.load_golden(path or FIX[name])
        self.B, self.T = self.z["grid0"].shape[0], self.z["actions"].shape[0]
        self._dev = {}

    def dev(self, key, t=None):
        """A recorded array (step t of a per-step one) on the device, cached."""
        k = (key, t)
        if k not in self._dev:
            a = self.z[key] if t is None else self.z[key][t]
            if a.dtype == np.uint64:
                a = a.view(np.int64)
            self._dev[k] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        return self._dev[k]

    def one_hot(self, t):
        k = ("one_hot", t)
        if k not in self._dev:
            self._dev[k] = torch.from_numpy(ob.one_hot(self.z["obs"][t])).to(DEV)
        return self._dev[k]

    @property
    def filled_boxes(self):
        z = self.z
        return bool(((z["grid0"][..., 0] == 7) & (z["grid0"][..., 2] >> 2 != 0)).any()
                    or ((z["agents0"][..., 5] == 7) & (z["agents0"][..., 7] >> 2 != 0)).any())

    def rep(self, a, N):
        """numpy [B_f, ...] -> [N, ...]: env n holds fixture env n % B_f"""
        return np.ascontiguousarray(np.take(a, np.arange(N) % self.B, axis=0))

    def env(self, N, cell_bytes=2, **kw):
        spec = dataclasses.replace(self.spec, cell_bytes=cell_bytes)
        e = BatchedMultiGridEnv(spec, N, DEV, **kw)
        z = self.z
        e.load_state(self.rep(z["grid0"], N), self.rep(z["agents0"], N), self.rep(z["rng0"], N),
                     self.rep(z["aux"], N) if spec.env_kind != "empty" else None, self.rep(z["step_count0"], N), validate=False)
        return e

    def actions(self, N, t=None):
        """i8[N,A] of step t, or i8[T,N,A] of every step, on the device"""
        a = self.z["actions"] if t is None else self.z["actions"][t]
        idx = np.arange(N) % self.B
        return torch.from_numpy(np.ascontiguousarray(a[:, idx] if t is None else a[idx])).to(DEV)


_FIXTURES = {}


def fixture(name) -> Fixture:
    if name not in _FIXTURES:
        _FIXTURES[name] = Fixture(name)
    return _FIXTURES[name]


def _same(got, want, B, ctx, what):
    """got [N, ...] on the device == want [B_f, ...] replicated; names the first env that differs"""
    N = got.shape[0]
    full, rest = divmod(N, B)
    g = got.reshape(N, -1)
    w = want.reshape(B, -1)
    if g.dtype == torch.float64:
        g, w = g.view(torch.int64), w.view(torch.int64)          # reward: bytes, not values
    ok = True
    if full:
        ok = bool((g[:full * B].view(full, B, -1) == w.unsqueeze(0)).all())
    if ok and rest:
        ok = bool((g[full * B:] == w[:rest]).all())
    if not ok:
        bad = (g != w[torch.arange(N, device=g.device) % B]).any(-1).nonzero()[:4].flatten().tolist()
        raise AssertionError(f"{ctx}: {what} differs from the reference's, envs {bad} (fixture envs {[n % B for n in bad]})")


def check_outputs(fx, t, outs, ctx, one_hot=False):
    obs, dr, rw, te, tr = outs[:5]
    B = fx.B
    _same(obs, fx.one_hot(t) if one_hot else fx.dev("obs", t), B, ctx, "one-hot obs" if one_hot else "obs")
    _same(dr, fx.dev("dir", t), B, ctx, "dir")
    _same(rw, fx.dev("reward", t), B, ctx, "reward")
    _same(te, fx.dev("terminated", t), B, ctx, "terminated")
    _same(tr, fx.dev("truncated", t), B, ctx, "truncated")


def check_state(fx, env, t, ctx):
    """the state after step t"""
    B = fx.B
    _same(env.grid, fx.dev("grid", t), B, ctx, "grid")
    _same(env.agents, fx.dev("agents", t), B, ctx, "agents")
    if fx.spec.num_agents > 1:
        _same(env.rng, fx.dev("rng", t), B, ctx, "rng")
    _same(env.step_count, fx.dev("step_count0") + (t + 1), B, ctx, "step_count")


def run_steps(fx, env, ctx, one_hot=False, T=None, state_every_step=True, **step_kw):
    N = env.batch
    for t in range(fx.T if T is None else T):
        outs = env.step(fx.actions(N, t), one_hot=one_hot, **step_kw)
        check_outputs(fx, t, outs, f"{ctx} step {t}", one_hot)
        if state_every_step or t == (fx.T if T is None else T) - 1:
            check_state(fx, env, t, f"{ctx} step {t}")
    env.check_errors()


def waves(spec, N):
    return -(-N // _lib.launch_info(spec, N)["envs_per_wavefront"])


@contextlib.contextmanager
def resident(ns):
    """Force a resident shape of the rollout / persistent launch (tests/test_resident.py): ns = 1 / 2 -> kShapes 7 / 8, 9 -> 9."""
    old = {k: os.environ.get(k) for k in ("MGX_RESIDENT_SHAPE", "MGX_RESIDENT_SLICES")}
    os.environ["MGX_RESIDENT_SHAPE"] = "9" if ns == 9 else ""
    os.environ["MGX_RESIDENT_SLICES"] = "" if ns == 9 else str(ns)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------------------------ the families

@pytest.mark.parametrize("name", util.RANDSTATE_IDS)
def test_latency_family(name):
    """One replica, then a ragged batch (3 replicas and a part of a fourth): gen_obs and every step."""
    fx = fixture(name)
    for N in (fx.B, 3 * fx.B + 5):
        env = fx.env(N)
        assert waves(env.spec, N) <= 2048
        obs, dr = env.gen_obs()
        _same(obs, fx.dev("obs0"), fx.B, f"{name} N={N} gen_obs", "obs")
        _same(dr, fx.dev("dir0"), fx.B, f"{name} N={N} gen_obs", "dir")
        run_steps(fx, env, f"{name} latency N={N}")


@pytest.mark.parametrize("name", util.RANDSTATE_IDS)
def test_throughput_family(name):
    """Enough replicas for more than 2048 wavefronts (launch_info, as test_throughput_instantiations_vs_oracle)."""
    fx = fixture(name)
    gw = _lib.launch_info(fx.spec, 1 << 16)["envs_per_wavefront"]
    N = 2049 * gw + 3
    env = fx.env(N)
    assert waves(env.spec, N) > 2048
    run_steps(fx, env, f"{name} throughput N={N}", state_every_step=False)


@pytest.mark.parametrize("name", util.RANDSTATE_IDS)
def test_one_hot_family(name):
    """The fused one-hot output == ob.one_hot (a plain numpy encoding) of the reference's recorded obs bytes; 16-bit cells, and
    compact cells where the fixture allows them (hook-free, no filled boxes)."""
    fx = fixture(name)
    N = 2 * fx.B + 7
    run_steps(fx, fx.env(N), f"{name} one-hot", one_hot=True)
    if fx.spec.env_kind == "empty" and not fx.filled_boxes:
        run_steps(fx, fx.env(N, cell_bytes=1), f"{name} compact one-hot", one_hot=True)


@pytest.mark.parametrize("name", util.RANDSTATE_IDS)
def test_compact_and_byte_grid_families(name):
    """cell_bytes = 1 (compact) and 3 (byte triples).  A fixture with filled boxes must be REFUSED by the compact format."""
    fx = fixture(name)
    N = 2 * fx.B + 3
    if fx.filled_boxes:
        with pytest.raises(ValueError, match="compact"):
            fx.env(N, cell_bytes=1)
    else:
        run_steps(fx, fx.env(N, cell_bytes=1), f"{name} compact")
    run_steps(fx, fx.env(N, cell_bytes=3), f"{name} byte grid")


@pytest.mark.parametrize("name", util.RANDSTATE_IDS)
def test_rollout_family(name):
    """mgx_rollout: every step of a [T, N, A] action script in one launch; the state written back at the end."""
    fx = fixture(name)
    N = 2 * fx.B + 9
    env = fx.env(N)
    out = env.rollout(fx.actions(N))
    for t in range(fx.T):
        check_outputs(fx, t, [out[k][t] for k in ("obs", "dir", "reward", "terminated", "truncated")], f"{name} rollout step {t}")
    check_state(fx, env, fx.T - 1, f"{name} rollout")
    env.check_errors()


# (fixture, batch, cell_bytes, kShapes entry of the plain step)
SHAPED = [(C24, 4096, 2, 1), (C24, 16384, 2, 2), (BUP, 16384, 2, 3), (C5, 32768, 2, 4), (C5, 36864, 1, 5), (C5, 32768, 1, 6)]


@pytest.mark.parametrize("name,N,cb,shape", SHAPED, ids=[f"shape{s[3]}" for s in SHAPED])
def test_shape_specialised_family(name, N, cb, shape):
    fx = fixture(name)
    env = fx.env(N, cell_bytes=cb)
    assert _lib.launch_info(env.spec, N)["fixed_shape"] == shape
    run_steps(fx, env, f"{name} shape {shape}", state_every_step=False)
    del env
    torch.cuda.empty_cache()


def test_specialise_family():
    """specialise(): a kernel compiled at run time (hipRTC) for a shape the library has none of."""
    fx = fixture("randstate_10x8_a3_v7_all_joint")
    N = 3 * fx.B + 1
    env = fx.env(N)
    assert env.specialise() in ("compiled", "registered")
    run_steps(fx, env, "specialise()")


def test_resident_rollout_family():
    """The resident rollout shapes of Empty-16x16 x 4 agents (kShapes 7 / 8 / 9), forced at small ragged batches."""
    fx = fixture(C24)
    for ns in (1, 2, 9):
        for N in (fx.B + 5, 3 * fx.B + 21):
            env = fx.env(N)
            with resident(ns):
                assert _lib.launch_info(env.spec, N, roll=True)["resident_shape"] == {1: 7, 2: 8, 9: 9}[ns]
                out = env.rollout(fx.actions(N))
            for t in range(fx.T):
                check_outputs(fx, t, [out[k][t] for k in ("obs", "dir", "reward", "terminated", "truncated")],
                              f"resident ns={ns} N={N} step {t}")
            check_state(fx, env, fx.T - 1, f"resident ns={ns} N={N}")
            env.check_errors()


@pytest.mark.parametrize("ns", [0, 1, 2])
def test_persistent_family(ns):
    """mgx_step_persistent on the 16x16 / A4 / v7 fixture: the plain launch (ns = 0) and the resident shapes 7 / 8."""
    fx = fixture(C24)
    N = 2 * fx.B + 11
    env = fx.env(N)
    with resident(ns) if ns else contextlib.nullcontext():
        with env.persistent(max_steps=fx.T) as ps:
            for t in range(fx.T):
                check_outputs(fx, t, ps.step(fx.actions(N, t)), f"persistent ns={ns} step {t}")
    assert ps.timeouts == 0 and ps.steps_completed == fx.T
    check_state(fx, env, fx.T - 1, f"persistent ns={ns}")
    env.check_errors()


@pytest.mark.parametrize("name", [C24, "randstate_9x6_a2_v5_noovl", BUP])
def test_sub_shard_chains(name):
    """capture_steps(sub_shards=P): P chains of T launches in one graph (the outputs of the last step, the state after it); and the
    eager step(sub_shards=P)."""
    fx = fixture(name)
    N = 8 * fx.B + 64
    for P in (2, 3):
        env = fx.env(N)
        acts = fx.actions(N)
        g = env.capture_steps(acts, sub_shards=P)
        assert g.sub_shards == P
        g.replay()
        torch.cuda.synchronize()
        t = fx.T - 1
        check_outputs(fx, t, (env.obs, env.dir, env.reward, env.terminated, env.truncated), f"{name} graph P={P}")
        check_state(fx, env, t, f"{name} graph P={P}")
        env = fx.env(N)
        for t in range(fx.T):
            env.step(fx.actions(N, t), sub_shards=P)
            env.join()
            check_outputs(fx, t, (env.obs, env.dir, env.reward, env.terminated, env.truncated), f"{name} eager P={P} step {t}")
        check_state(fx, env, fx.T - 1, f"{name} eager P={P}")
        env.check_errors()


# -------------------------------------------------------------------------------------- the reward at every step count (base.py:602)

MAX_STEPS = sorted(set(range(1, 65)) | {67, 97, 101, 127, 251, 509, 1021, 4093, 8191, 65521, 1000, 1024, 4096, 16384, 65535, 1 << 20})


def _reward_envs(M, A, joint):
    """One env per step count in [0, M) (a strided sample of ~4096 for large M): A agents in a row of a 5-high grid, each facing a
    goal one cell to its right.  Returns (spec, grid, agents, step_count, the expected reward f64[N, A])."""
    sc = np.arange(M, dtype=np.int64)
    if M > 4096:
        sc = np.unique(np.concatenate([np.arange(0, M, -(-M // 4096)), np.arange(M - 64, M), np.arange(64)]))
    N = len(sc)
    spec = EnvSpec(4, 2 + A, A, 3, max_steps=M, joint_reward=joint, success_termination_mode="all")
    grid = np.zeros((N, 2 + A, 4, 3), np.uint8)
    grid[..., 0] = 1
    grid[:, 0], grid[:, -1], grid[:, :, 0], grid[:, :, -1] = (2, 5, 0), (2, 5, 0), (2, 5, 0), (2, 5, 0)
    grid[:, 1:1 + A, 2] = (8, 1, 0)
    agents = np.zeros((N, A, 8), np.uint8)
    agents[..., 0] = np.arange(A) % 6
    agents[..., 2] = 1
    agents[..., 3] = 1 + np.arange(A)
    agents[..., 5] = 1
    # multigrid/base.py:333 (step_count += 1 first), 598-602: 1 - 0.9 * (step_count / max_steps) in Python float (IEEE double)
    r = 1 - 0.9 * ((sc + 1).astype(np.float64) / np.float64(M))
    return spec, grid, agents, sc.astype(np.int32), np.repeat(r[:, None], A, axis=1)


def test_reward_at_every_step_count():
    """The kernels' __ddiv_rn / __dmul_rn / __dsub_rn against the reference's expression evaluated in float64 by numpy, at every step
    count of each max_steps; one agent, and three agents succeeding in the same step (own and joint rewards: the reference ASSIGNS
    the same value to every agent, base.py:502-505); the plain step, the one-hot step and the fused auto-reset step."""
    checked = 0
    for M in MAX_STEPS:
        for A, joint in ((1, False), (3, False), (3, True)):
            spec, grid, agents, sc, want = _reward_envs(M, A, joint)
            N = grid.shape[0]
            wt = torch.from_numpy(want).to(DEV).view(torch.int64)
            for mode in ("plain", "one_hot", "auto_reset"):
                env = BatchedMultiGridEnv(spec, N, DEV)
                env.load_state(grid, agents, np.tile(np.array([1, 2, 3, 5], np.uint64), (N, 1)), None, sc)
                if mode == "auto_reset":
                    env.set_layout_pool(grid[:1], agents[:1])
                acts = torch.full((N, A), 2, dtype=torch.int8, device=DEV)
                out = env.step(acts, one_hot=mode == "one_hot", auto_reset=mode == "auto_reset")
                got = out[2].view(torch.int64)
                if not torch.equal(got, wt):
                    bad = (got != wt).any(-1).nonzero()[:4].flatten().tolist()
                    g = out[2].cpu().numpy()
                    raise AssertionError(f"max_steps={M} A={A} joint={joint} {mode}: step counts {[int(sc[b]) for b in bad]} "
                                         f"give {[g[b, 0].hex() for b in bad]}, want {[want[b, 0].hex() for b in bad]}")
                assert bool((out[3] == 1).all()), (M, A, joint, mode)
                assert torch.equal(out[4].cpu(), torch.from_numpy((sc + 1 >= M).astype(np.uint8))), (M, A, joint, mode)
                if mode == "auto_reset":
                    assert int(env.was_reset.sum()) == 0
                checked += N
    assert checked > 100_000


# ------------------------------------------------------------------------------------------------------------ bounds-checked build

def test_bounds_checked_build_counts_no_violation():
    """Only meaningful inside the bounds-checked run below (MGX_LIBMGX = libmgx_chk.so): after every test of this file, no LDS
    access left its wavefront's slice."""
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
