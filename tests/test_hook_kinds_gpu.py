"""RedBlueDoors, LockedHallway (explicit and geometric aux) and the declared `rules` kind through every kernel family the ABI accepts
for them.  The matrix tests elsewhere (tests/test_instantiations.py, the randstate_bup_* fixture) use BlockedUnlockPickup wherever
they set hooks -- the one hook that reads no tile, writes no aux, ignores hook_order and assigns its rewards; the other kinds are
run-time branches inside the same instantiations, so coverage by kernel name says nothing about them.

Two sources of truth, everything compared bit for bit (obs or its one-hot bytes, dir, reward bytes, terminated, truncated; the grid,
agents, generator words, step_count and all 16 aux bytes; was_reset and episode where there is a reset):
  * the REFERENCE's recorded bytes: every rbd_* / lh_* fixture of tests/golden, replicated along the batch.  The fixtures do not
    record the hook state itself (it lives in Python attributes of the reference's env), so the expected aux is the oracle's along the
    same fixture -- whose outputs and state are first required to equal the recorded ones;
  * the ORACLE on the hook-dense cases of tests/hook_states.py (their density is asserted on the CPU, tests/test_hook_states.py):
    512 base envs, env n of a launch holds base env n % 512, so ONE vectorised compare on the device checks every env of a batch
    however big -- not three slices of it.

The whole file runs once more on the bounds-checked build (the last test)."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, _lib, layouts
from oracle import binding as ob
from tests import hook_states as hs
from tests import util
from tests.test_reference_random_states_gpu import _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("obs", "dir", "reward", "terminated", "truncated")
STATE = ("grid", "agents", "rng", "step_count", "aux")
#: one case per kind and aux format for the families that cost a launch sequence each; the step families take every case
MAIN = ["rbd_a3_all_v3", "rbd_a2_any_v9", "lh2_a2_own_v7", "lh8_a4_joint_v7", "lh12_a3_own_v7", "rules_fetchtrap_a2_v7"]
ORDERED = [n for n in hs.NAMES if hs.kind_of(n) != "rules"]
#: (case, with its visiting-order script?) -- the rules cases have no script: their ascending run is the whole test
RUNS = [(n, o) for n in hs.NAMES for o in (True, False) if o is False or n in ORDERED]
RUN_IDS = [f"{n}-{'hook_order' if o else 'ascending'}" for n, o in RUNS]


def _t(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


class Ref:
    """A run of B base envs (a list over the steps of dicts of numpy arrays: outputs and post-step state), on the device, cached."""

    def __init__(self, steps, B):
        self.steps, self.B, self._dev = steps, B, {}

    def dev(self, key, t):
        k = (key, t)
        if k not in self._dev:
            self._dev[k] = _t(ob.one_hot(self.steps[t]["obs"]) if key == "one_hot" else self.steps[t][key])
        return self._dev[k]

    def check_outputs(self, t, outs, ctx, one_hot=False):
        _same(outs[0], self.dev("one_hot" if one_hot else "obs", t), self.B, ctx, "one-hot obs" if one_hot else "obs")
        for k, x in zip(OUT[1:], outs[1:5]):
            _same(x, self.dev(k, t), self.B, ctx, k)

    def check_state(self, t, env, ctx, extra=()):
        for k in STATE + tuple(extra):
            _same(getattr(env, k), self.dev(k, t), self.B, ctx, k)


_REFS = {}


def ref(name, ordered=True) -> Ref:
    ordered = ordered and hs.case(name).hook_order is not None
    if (name, ordered) not in _REFS:
        _REFS[name, ordered] = Ref(hs.trajectory(name, ordered), hs.BASE)
    return _REFS[name, ordered]


def rep(a, N, B=hs.BASE):
    return np.ascontiguousarray(np.take(a, np.arange(N) % B, axis=0))


def make_env(name, N, cell_bytes=2, state=None, **kw):
    c = hs.case(name)
    st = state or c.state
    env = BatchedMultiGridEnv(dataclasses.replace(c.spec, cell_bytes=cell_bytes), N, DEV, **kw)
    env.load_state(rep(st["grid"], N), rep(st["agents"], N), rep(st["rng"], N), rep(st["aux"], N), rep(st["step_count"], N), validate=False)
    return env


_SCRIPTS = {}


def script(name, N, what="actions", t=None):
    """i8[T,N,A] actions / u8[T,N,A] visiting orders of the case on the device (step t of it), env n = base env n % 512"""
    k = (name, N, what)
    if k not in _SCRIPTS:
        a = getattr(hs.case(name), what)
        _SCRIPTS[k] = None if a is None else _t(np.take(a, np.arange(N) % hs.BASE, axis=1))
    s = _SCRIPTS[k]
    return s if (t is None or s is None) else s[t]


def outs_of(env, one_hot=False):
    return (env._one_hot if one_hot else env.obs), env.dir, env.reward, env.terminated, env.truncated


def run_steps(name, env, ctx, ordered=True, one_hot=False, T=None, state_every_step=True, **kw):
    N, rf = env.batch, ref(name, ordered)
    T = hs.T_STEPS if T is None else T
    for t in range(T):
        outs = env.step(script(name, N, t=t), one_hot=one_hot, hook_order=script(name, N, "hook_order", t) if ordered else None, **kw)
        if kw.get("sub_shards", 1) != 1:
            env.join()
        rf.check_outputs(t, outs, f"{ctx} step {t}", one_hot)
        if state_every_step or t == T - 1:
            rf.check_state(t, env, f"{ctx} step {t}")
    env.check_errors()


def waves(spec, N):
    return -(-N // _lib.launch_info(spec, N)["envs_per_wavefront"])


def rollout_ordered(env, acts, order, auto_reset=False, one_hot=False):
    """mgx_step_ex with steps = T and a [T,B,A] hook_order script (BatchedMultiGridEnv.rollout has no parameter for it); returns the
    C ABI's code and the outputs."""
    sp, B, T = env.spec, env.batch, acts.shape[0]
    A, v = sp.num_agents, sp.view_size
    out = {"obs": torch.empty((T, B, A, v, v, 21 if one_hot else 3), dtype=torch.uint8, device=DEV),
           "dir": torch.empty((T, B, A), dtype=torch.uint8, device=DEV), "reward": torch.empty((T, B, A), dtype=torch.float64, device=DEV),
           "terminated": torch.empty((T, B, A), dtype=torch.uint8, device=DEV), "truncated": torch.empty((T, B), dtype=torch.uint8, device=DEV)}
    ar = None
    if auto_reset:
        out["was_reset"] = torch.empty((T, B), dtype=torch.uint8, device=DEV)
        ar = env._auto_reset_args(True, out["was_reset"])
    sa, keep = env.backend.step_args(env.cells, env.agents, env.rng, env.step_count, env.aux, env.err, out["obs"], out["dir"],
                                     out["reward"], out["terminated"], out["truncated"], auto_reset=ar, one_hot=one_hot)
    sa.steps, sa.actions = T, acts.data_ptr()
    sa.hook_order = order.data_ptr() if order is not None else None
    with torch.cuda.device(env.device):
        rc = _lib.lib().mgx_step_ex(C.byref(env.backend.sc), B, C.byref(sa), torch.cuda.current_stream(env.device).cuda_stream)
    torch.cuda.synchronize()
    return rc, out


# ------------------------------------------------------------------------------------------- the reference's recorded bytes

HOOK_FIXTURES = [p for p in util.GOLDEN if os.path.basename(p).startswith(("rbd_", "lh_"))]


def _fixture_ref(path):
    """(spec, initial state, actions [T,1,A], orders or None, Ref) of a single-env rollout fixture in the product's layout"""
    z, d, spec = util.load_golden(path)
    T = z["actions"].shape[0]
    st = dict(grid=layouts.grid_to_product(z["grid0"])[None], agents=layouts.pack_agents(z["agents0"])[None],
              rng=util.rng_words_lohi(z["rng0"])[None], step_count=np.zeros(1, np.int32), aux=util.golden_aux(d)[None])
    orders = z["hook_order"][:, None].astype(np.uint8) if "hook_order" in z.files else None
    cur = {k: v.copy() for k, v in st.items()}
    steps = []
    for t in range(T):
        o = ob.step_batch(spec.as_dict(), cur["grid"], cur["agents"], cur["rng"], cur["step_count"], np.ascontiguousarray(z["actions"][t][None]),
                          cur["aux"], hook_order=None if orders is None else np.ascontiguousarray(orders[t]))
        rec = dict(obs=z["obs"][t][None], dir=z["direction"][t][None].astype(np.uint8), reward=z["reward"][t][None],
                   terminated=z["terminated"][t][None].astype(np.uint8), truncated=np.array([z["truncated"][t]], np.uint8),
                   grid=layouts.grid_to_product(z["grid"][t])[None], agents=layouts.pack_agents(z["agents"][t])[None])
        for k, x in zip(OUT, o):                                  # the oracle stands in for the unrecorded aux only where it
            assert np.asarray(x).tobytes() == np.ascontiguousarray(rec[k]).astype(x.dtype).tobytes(), (path, t, k)   # reproduces the rest
        assert np.array_equal(cur["grid"], rec["grid"]) and np.array_equal(cur["agents"], rec["agents"]), (path, t)
        rec.update(rng=cur["rng"].copy(), step_count=cur["step_count"].copy(), aux=cur["aux"].copy())
        steps.append({k: np.ascontiguousarray(v) for k, v in rec.items()})
    assert np.array_equal(cur["rng"][0], util.rng_words_lohi(z["rng_final"]))
    return spec, st, z["actions"][:, None].astype(np.int8), orders, Ref(steps, 1)


@pytest.mark.parametrize("path", HOOK_FIXTURES, ids=[os.path.basename(p)[:-4] for p in HOOK_FIXTURES])
def test_reference_fixtures_latency_throughput_and_rollout(path):
    """Every recorded RedBlueDoors / LockedHallway rollout, replicated: the latency step at a ragged batch, the throughput step
    (more than 2048 wavefronts) and the rollout with the recorded visiting orders.  The first 12 steps of each: the scripted
    fixtures do their unlocks, failures and order-dependent steps within their first 8, the rest is a random tail (which
    test_golden_replay steps in full), and the random fixtures are walks that barely reach a hook; 12 steps keep each case to well
    under a second.  The throughput batch compares its outputs every step and its state after the last one."""
    spec, st, acts, orders, rf = _fixture_ref(path)
    T = min(12, acts.shape[0])
    gw = _lib.launch_info(spec, 1 << 16)["envs_per_wavefront"]
    for N, fam in ((133, "latency"), (2049 * gw + 3, "throughput")):
        assert (waves(spec, N) > 2048) == (fam == "throughput")
        env = BatchedMultiGridEnv(spec, N, DEV)
        env.load_state(*(rep(st[k], N, 1) for k in ("grid", "agents", "rng", "aux", "step_count")), validate=False)
        for t in range(T):
            outs = env.step(_t(rep(acts[t], N, 1)), hook_order=None if orders is None else _t(rep(orders[t], N, 1)))
            rf.check_outputs(t, outs, f"{fam} step {t}")
            if fam == "latency" or t == T - 1:
                rf.check_state(t, env, f"{fam} step {t}")
        env.check_errors()
    N = 77
    env = BatchedMultiGridEnv(spec, N, DEV)
    env.load_state(*(rep(st[k], N, 1) for k in ("grid", "agents", "rng", "aux", "step_count")), validate=False)
    a = _t(np.take(acts[:T], np.zeros(N, np.int64), axis=1))
    o = None if orders is None else _t(np.take(orders[:T], np.zeros(N, np.int64), axis=1))
    rc, out = rollout_ordered(env, a, o)
    assert rc == 0
    for t in range(T):
        rf.check_outputs(t, [out[k][t] for k in OUT], f"rollout step {t}")
    rf.check_state(T - 1, env, "rollout")
    env.check_errors()


# ---------------------------------------------------------------------------------------------------- the oracle, hook-dense

@pytest.mark.parametrize("name,ordered", RUNS, ids=RUN_IDS)
def test_latency_and_throughput_families(name, ordered):
    """The latency step at a ragged batch of a few hundred envs, then the same case beyond 2048 wavefronts with a ragged last one."""
    c = hs.case(name)
    gw = _lib.launch_info(c.spec, 1 << 16)["envs_per_wavefront"]
    for N, fam in ((hs.BASE + 37, "latency"), (2049 * gw + 3, "throughput")):
        assert (waves(c.spec, N) > 2048) == (fam == "throughput")
        run_steps(name, make_env(name, N), f"{name} {fam} N={N}", ordered, state_every_step=fam == "latency",
                  T=None if fam == "latency" else 6)


def test_streamed_family():
    """The smallest grid of the builder (LockedHallway, 2 rooms: 13 x 5) at a batch whose grid tensor just exceeds 128 MiB: streamed
    tile loads.  With the visiting-order script."""
    name = "lh2_a2_own_v7"
    sp = hs.case(name).spec
    assert sp.width * sp.height == min(hs.case(n).spec.width * hs.case(n).spec.height for n in hs.NAMES)
    N = (128 << 20) // (sp.width * sp.height * 2) + 1
    env = make_env(name, N)
    nbytes = env.cells.numel() * env.cells.element_size()
    assert (128 << 20) < nbytes <= (128 << 20) + sp.width * sp.height * 2
    run_steps(name, env, f"{name} streamed N={N}", True, state_every_step=False, T=3)
    del env
    _SCRIPTS.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", hs.NAMES)
def test_compact_and_byte_grid_families(name):
    """cell_bytes 1 and 3: the plain step with the visiting orders; the one-hot step and the rollout are refused."""
    N = hs.BASE + 3
    for cb in (1, 3):
        env = make_env(name, N, cell_bytes=cb)
        run_steps(name, env, f"{name} cell_bytes={cb}", True)
        acts = script(name, N)
        with pytest.raises(NotImplementedError):
            env.step(acts[0], one_hot=True)
        with pytest.raises(NotImplementedError):
            env.rollout(acts)
        # ... and by the C ABI itself, with the documented code
        rc, _ = rollout_ordered(env, acts, script(name, N, "hook_order"))
        assert rc == _lib.ERR_UNSUPPORTED, (name, cb, rc)
        oh = torch.zeros(tuple(env.obs.shape[:-1]) + (21,), dtype=torch.uint8, device=DEV)
        with pytest.raises(_lib.MgxError) as e:
            env.backend.step(N, env.cells, env.agents, env.rng, env.step_count, acts[0], env.aux, env.err, oh, env.dir, env.reward,
                             env.terminated, env.truncated, one_hot=True)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        ref(name).check_state(hs.T_STEPS - 1, env, f"{name} cell_bytes={cb}: the refused launches must not touch the state")


@pytest.mark.parametrize("name", hs.NAMES)
def test_one_hot_family(name):
    run_steps(name, make_env(name, hs.BASE + 9), f"{name} one-hot", True, one_hot=True)


@pytest.mark.parametrize("name,ordered", RUNS, ids=RUN_IDS)
def test_rollout_family(name, ordered):
    """mgx_rollout with a [T,B,A] visiting-order script and without one: every step's outputs; aux (kept in LDS over the launch)
    after the launch == aux after T steps; a second rollout continues from the written-back state."""
    N, T1 = hs.BASE + 21, 6
    rf = ref(name, ordered)
    env = make_env(name, N)
    acts, order = script(name, N), script(name, N, "hook_order") if ordered else None
    for lo, hi in ((0, T1), (T1, hs.T_STEPS)):
        a = acts[lo:hi].contiguous()
        if ordered:
            rc, out = rollout_ordered(env, a, order[lo:hi].contiguous())
            assert rc == 0
        else:
            out = env.rollout(a)
        for t in range(lo, hi):
            rf.check_outputs(t, [out[k][t - lo] for k in OUT], f"{name} rollout step {t}")
        rf.check_state(hi - 1, env, f"{name} rollout after step {hi - 1}")
    env.check_errors()


@pytest.mark.parametrize("name", MAIN)
def test_persistent_family(name):
    """mgx_step_persistent refuses a visiting order (asserted), so: ascending order, the outputs of every step, the state -- aux
    included -- written back when the launch closes."""
    N = hs.BASE + 11
    env = make_env(name, N)
    rf = ref(name, False)
    sa = _lib.MgxStepArgs()
    sa.steps = 1
    sa.hook_order = script(name, N, "actions", 0).data_ptr()              # (any non-null pointer: refused before it is read)
    out = C.c_int32(0)
    with torch.cuda.device(env.device):
        assert _lib.lib().mgx_persistent_waves(C.byref(env.backend.sc), N, C.byref(sa), C.byref(out)) == _lib.ERR_UNSUPPORTED
    with env.persistent(max_steps=hs.T_STEPS) as ps:
        for t in range(hs.T_STEPS):
            rf.check_outputs(t, ps.step(script(name, N, t=t)), f"{name} persistent step {t}")
    assert ps.timeouts == 0 and ps.steps_completed == hs.T_STEPS
    rf.check_state(hs.T_STEPS - 1, env, f"{name} persistent")
    env.check_errors()


# ------------------------------------------------------------------------------------------ fused auto-reset with pool_aux

K_POOL = 8          # divides 512: the pool index (first_env + n + episode * 7919) % K of env n is that of base env n % 512


def _ar_case(name):
    """The case with envs that restart inside the run -- step_count at max_steps - 1 (every 4th env) or all agents terminated (the
    next one), whatever their stale flag / unlocked mask, and the forced-termination byte set in some -- and a pool of fresh
    layouts whose aux differs: stale flag clear, mask zero, aux[15] zero."""
    c = hs.case(name)
    st = {k: v.copy() for k, v in c.state.items()}
    b = np.arange(hs.BASE)
    st["step_count"][b % 4 == 0] = c.spec.max_steps - 1
    st["agents"][b % 4 == 1, :, 4] = 1
    kind = hs.kind_of(name)
    if kind == "lockedhallway":
        st["aux"][b % 8 == 1, 15] = 1
        geo = (c.state["aux"][:, 0] & 0x80) != 0                           # (explicit format: aux[2] is a door's x, not mask bits)
        fresh = (c.state["aux"][:, 1] == 0) & ((c.state["aux"][:, 2] == 0) | ~geo)
    elif kind == "redbluedoors":
        fresh = c.state["aux"][:, 4] == 0
    else:
        fresh = np.ones(hs.BASE, bool)
    pick = np.nonzero(fresh & (c.state["agents"][:, :, 4] == 0).all(1))[0][:K_POOL]
    assert len(pick) == K_POOL
    pool = tuple(c.state[k][pick].copy() for k in ("grid", "agents", "aux"))
    return c, st, pool


_AR_REFS = {}


def ar_ref(name, ordered):
    """reset_done followed by the step, on the oracle backend: outputs, state, was_reset and episode after every step"""
    ordered = ordered and hs.case(name).hook_order is not None
    if (name, ordered) not in _AR_REFS:
        c, st, pool = _ar_case(name)
        env = BatchedMultiGridEnv(c.spec, hs.BASE, "cpu", backend=util.OracleBackend(c.spec, nthreads=4))
        env.load_state(st["grid"], st["agents"], st["rng"], st["aux"], st["step_count"], validate=False)
        env.set_layout_pool(*pool)
        steps = []
        for t in range(hs.T_STEPS):
            o = env.step(torch.from_numpy(np.ascontiguousarray(c.actions[t])), auto_reset=True,
                         hook_order=torch.from_numpy(np.ascontiguousarray(c.hook_order[t])) if ordered else None)
            rec = {k: x.numpy().copy() for k, x in zip(OUT, o)}
            rec.update({k: getattr(env, k).numpy().copy() for k in STATE + ("was_reset", "episode")})
            steps.append(rec)
        assert sum(int(s["was_reset"].sum()) for s in steps) > hs.BASE // 2
        _AR_REFS[name, ordered] = Ref(steps, hs.BASE)
    return _AR_REFS[name, ordered]


def _ar_env(name, N):
    c, st, pool = _ar_case(name)
    env = make_env(name, N, state=st)
    env.set_layout_pool(*pool)
    return env


@pytest.mark.parametrize("form", ["step", "step_one_hot", "rollout", "rollout_one_hot", "persistent"])
@pytest.mark.parametrize("name", MAIN)
def test_fused_auto_reset_from_a_pool_with_aux(name, form):
    """The restart must bring the pool layout's aux along (stale flag, unlocked mask, forced-termination byte): as the step (with the
    visiting orders), as the rollout (with and without them), as the persistent launch, and with the one-hot output."""
    N = hs.BASE + 5
    one_hot = form.endswith("one_hot")
    if form.startswith("step"):
        env, rf = _ar_env(name, N), ar_ref(name, True)
        for t in range(hs.T_STEPS):
            outs = env.step(script(name, N, t=t), auto_reset=True, one_hot=one_hot, hook_order=script(name, N, "hook_order", t))
            rf.check_outputs(t, outs, f"{name} {form} step {t}", one_hot)
            rf.check_state(t, env, f"{name} {form} step {t}", extra=("was_reset", "episode"))
    elif form.startswith("rollout"):
        for ordered in (True, False):
            env, rf = _ar_env(name, N), ar_ref(name, ordered)
            if ordered and hs.case(name).hook_order is not None:
                rc, out = rollout_ordered(env, script(name, N), script(name, N, "hook_order"), auto_reset=True, one_hot=one_hot)
                assert rc == 0
            else:
                out = env.rollout(script(name, N), auto_reset=True, one_hot=one_hot)
            for t in range(hs.T_STEPS):
                rf.check_outputs(t, [out[k][t] for k in OUT], f"{name} {form} ordered={ordered} step {t}", one_hot)
                _same(out["was_reset"][t], rf.dev("was_reset", t), hs.BASE, f"{name} {form} step {t}", "was_reset")
            rf.check_state(hs.T_STEPS - 1, env, f"{name} {form} ordered={ordered}", extra=("episode",))
    else:
        env, rf = _ar_env(name, N), ar_ref(name, False)
        with env.persistent(max_steps=hs.T_STEPS, auto_reset=True) as ps:
            for t in range(hs.T_STEPS):
                rf.check_outputs(t, ps.step(script(name, N, t=t)), f"{name} persistent auto-reset step {t}")
                _same(env.was_reset, rf.dev("was_reset", t), hs.BASE, f"{name} persistent step {t}", "was_reset")
        assert ps.timeouts == 0 and ps.steps_completed == hs.T_STEPS
        rf.check_state(hs.T_STEPS - 1, env, f"{name} persistent auto-reset", extra=("episode",))
    env.check_errors()


# ------------------------------------------------------------------------------------- sub-shard chains, specialise, generation

@pytest.mark.parametrize("name", [n for n in MAIN if n in ORDERED])
def test_sub_shard_chains_slice_the_visiting_orders(name):
    """capture_steps(sub_shards=P) and the eager step(sub_shards=P), P = 2 and 3, on a batch that does not divide evenly: every
    chain must read ITS block of the [T,B,A] visiting-order script."""
    N = 3 * hs.BASE + 64 + 37
    rf = ref(name)
    for P in (2, 3):
        env = make_env(name, N)
        g = env.capture_steps(script(name, N), sub_shards=P, hook_order=script(name, N, "hook_order"))
        assert g.sub_shards == P
        g.replay()
        torch.cuda.synchronize()
        rf.check_outputs(hs.T_STEPS - 1, outs_of(env), f"{name} graph P={P}")
        rf.check_state(hs.T_STEPS - 1, env, f"{name} graph P={P}")
        env.check_errors()
        run_steps(name, make_env(name, N), f"{name} eager P={P}", True, state_every_step=False, sub_shards=P)


@pytest.mark.parametrize("name", ["rbd_a3_all_v3", "lh12_a3_own_v7"])
def test_specialise_family(name):
    """specialise(): the kernel compiled at run time (hipRTC) for exactly this shape."""
    env = make_env(name, hs.BASE + 1)
    assert env.specialise() in ("compiled", "registered")
    run_steps(name, env, f"{name} specialise()", True)


GENERATED = [("rbd_a3_all_v3", dict(kind="redbluedoors")), ("lh2_a2_own_v7", dict(kind="lockedhallway", room_size=5)),
             ("lh8_a4_joint_v7", dict(kind="lockedhallway", room_size=4)), ("lh12_a3_own_v7", dict(kind="lockedhallway", room_size=4))]


def _stand_at_generated_doors(kind, grid, agents, aux, r):
    """New agent rows u8[B,A,8] for GENERATED episodes: every agent beside a door whose place is read from the env's generated aux,
    facing it -- LockedHallway: from the hallway, holding the key of the door's colour (read from the generated grid); RedBlueDoors:
    inside the middle room, agents in turn at the red and the blue door.  An agent whose cell is taken by an object stays put."""
    out = agents.copy()
    B, A = agents.shape[:2]
    for b in range(B):
        x = aux[b]
        if kind == "redbluedoors":
            doors = [(int(x[2]), int(x[3]), 1), (int(x[0]), int(x[1]), -1)]             # (x, y, the side the room is on)
        elif x[0] & 0x80:
            rs = int(x[3])
            doors = [((rs - 1) * (1 + k % 2), (k // 2) * (rs - 1) + (rs - 1) // 2, 1 if k % 2 == 0 else -1) for k in range(x[0] & 0x7f)]
        else:
            doors = [(int(x[2 + 2 * k]), int(x[3 + 2 * k]), 1 if x[2 + 2 * k] < grid.shape[2] // 2 else -1) for k in range(x[0])]
        pick = r.permutation(len(doors))
        for a in range(A):
            dx, dy, side = doors[pick[a % len(doors)]]
            assert grid[b, dy, dx, 0] == hs.DOOR, "the generated aux does not name a door"
            if grid[b, dy, dx + side, 0] != 1:
                continue
            out[b, a, 1:5] = (2 if side == 1 else 0, dx + side, dy, 0)
            if kind == "lockedhallway":
                out[b, a, 5:8] = (hs.KEY, grid[b, dy, dx, 1], 0)
    return out


@pytest.mark.parametrize("name,gen", GENERATED, ids=[g[0] for g in GENERATED])
def test_device_generation_then_hooks(name, gen):
    """mgx_step_generate: the episodes that end are regenerated on the device; the point here is the steps AFTER an adoption -- the
    generated aux (door positions, a zero mask, a clear stale flag) is what the hook then reads.  A generated episode starts with
    empty-handed agents anywhere and lasts 6 steps here, so a walk would never reach a hook: once every env has been regenerated
    (and again two episodes later) the same agent rows are written into both envs -- every agent beside a door named by the GENERATED
    aux, LockedHallway agents holding its key.  Against OracleBackend.step + reset_generate, every output and the state each step.
    Asserted on the oracle's side: at least 32 of the 192 envs reach a hook event in a generated episode (RedBlueDoors: a success or the
    stale flag set; LockedHallway: the unlocked mask gains a bit)."""
    c = hs.case(name)
    kind = hs.kind_of(name)
    spec = dataclasses.replace(c.spec, max_steps=6)
    B, T = 192, 20
    envs = []
    for dev, kw in ((DEV, {}), ("cpu", dict(backend=util.OracleBackend(spec, nthreads=4)))):
        e = BatchedMultiGridEnv(spec, B, dev, first_env=17, **kw)
        st = c.state
        e.load_state(st["grid"][:B], st["agents"][:B], st["rng"][:B], st["aux"][:B], np.minimum(st["step_count"][:B], 5), validate=False)
        e.set_layout_generator(layout_seed=11, **gen)
        envs.append(e)
    hip, cpu = envs
    r = np.random.default_rng(5)
    reached = np.zeros(B, bool)
    geo = bool(c.state["aux"][0, 0] & 0x80)

    def mask(aux):
        return aux[:, 1].astype(np.int64) | ((aux[:, 2].astype(np.int64) << 8) if geo else 0)

    for t in range(T):
        if t in (7, 14):
            assert int(cpu.episode.min()) >= 1
            rows = torch.from_numpy(_stand_at_generated_doors(kind, cpu.grid.numpy(), cpu.agents.numpy(), cpu.aux.numpy(), r))
            cpu.agents.copy_(rows)
            hip.agents.copy_(rows.to(DEV))
        act = torch.from_numpy(r.choice(np.array([5, 5, 5, 2, 0, 1, 6], np.int8), size=(B, spec.num_agents)))
        order = torch.from_numpy(np.argsort(r.random((B, spec.num_agents)), axis=-1).astype(np.uint8))
        pre = cpu.aux.numpy().copy()
        generated = cpu.episode.numpy() > 0
        got = hip.step(act.to(DEV), auto_reset=True, hook_order=order.to(DEV))
        want = [x.clone() for x in cpu.step(act, hook_order=order)]
        post = cpu.aux.numpy()
        if kind == "redbluedoors":
            reached |= generated & ((want[2].numpy() > 0).any(1) | ((pre[:, 4] == 0) & (post[:, 4] == 1)))
        else:
            reached |= generated & ((mask(post) & ~mask(pre)) != 0) & (want[2].numpy() > 0).any(1)
        cpu.reset_done()
        for k, (g, w) in zip(OUT, zip(got, want)):
            assert g.cpu().numpy().tobytes() == w.numpy().tobytes(), f"{name} generate step {t}: {k}"
        for f in ("was_reset", "grid", "agents", "rng", "step_count", "aux", "episode"):
            assert torch.equal(getattr(hip, f).cpu(), getattr(cpu, f)), f"{name} generate step {t}: {f}"
    assert int(cpu.episode.min()) >= 2
    print(f"{name}: {int(reached.sum())} of {B} envs reach a hook event in a generated episode")
    assert reached.sum() >= 32, f"{name}: only {int(reached.sum())} envs reach a hook event in a generated episode"
    hip.check_errors()


# ------------------------------------------------------------------------------------------------------------ bounds-checked build

def test_bounds_checked_build_counts_no_violation():
    """Only meaningful inside the bounds-checked run below (MGX_LIBMGX = libmgx_chk.so)."""
    from multigrid_amd import build
    if os.environ.get("MGX_LIBMGX") != build.LIB_CHK:
        return
    v = (C.c_int32 * 2)()
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
