"""Every form a REGISTERED shape serves (multigrid_amd/jit.py; choose_in_family in csrc/mgx_fused.h).  `jit.source_for` emits two kernels
per shape, and once a geometry is registered every plain-step launch of it with auto-reset runs the second, `mgx_jit_step_ar`: the
restart, the `pool_aux` copy and the layout marker's stores, compiled by hipRTC.  tests/test_jit_shapes.py and the
`test_specialise_family` tests step without auto-reset; here the registered kernel runs

  * with auto-reset from a pool of three layouts at first_env = 11, a quarter of the envs one step from truncation and a quarter with
    every agent terminated, on ragged batches (one of a single wavefront), against the oracle backend after every one of 10 steps;
  * on two hook envs with `pool_aux` and the visiting orders (the cases and the reference of tests/test_hook_kinds_gpu.py);
  * under stream capture -- capture_steps(auto_reset=True), one chain, replayed twice;
  * behind the composite launcher of track_episodes(), the books against the sequential model over the recorded outputs;
  * through a random call sequence: the forms `plain_jit` and `pool1_jit` of tests/env_sequences.py, which have these two shapes, in
    tests/test_env_sequences_gpu.py;
  * as a THROUGHPUT kernel that reads the layout marker: ensure_shape(latency_only=False) at the smallest batch of more than 2048
    wavefronts, then the parity and the read-is-taken checks of tests/test_marker_sizes_gpu.py.
A registration lasts for the process and serves every env of its geometry, so the hook-free shapes here -- 7x6 x 3 agents view 5,
6x5 x 2 agents view 3, 8x8 x 2 agents view 5 at the throughput batch -- are used by no other test file; the two hook cases are those
`test_specialise_family` of tests/test_hook_kinds_gpu.py registers anyway.  Five hipRTC keys in all; every test first asserts that
launch_info reports MGX_SHAPE_RUNTIME_COMPILED (100) for its batch."""
import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib, jit
from tests import env_sequences as es
from tests import hook_states as hs
from tests import marker_sizes as ms
from tests import test_hook_kinds_gpu as hk
from tests import util
from tests.test_episode_stats import BEFORE, assert_same as assert_same_books, model_stats, new_state, record, snapshot
from tests.test_grid_layout_marker import holds
from tests.test_marker_sizes_gpu import check_parity, check_read

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not jit.hiprtc_available(), reason="no libhiprtc")]
DEV = "cuda:0"
RUNTIME_COMPILED = 100                                        # include/mgx.h: MGX_SHAPE_RUNTIME_COMPILED
SPEC_A, SPEC_B = EnvSpec(7, 6, 3, 5, max_steps=6), EnvSpec(6, 5, 2, 3, max_steps=6)
OUT = ("obs", "dir", "reward", "terminated", "truncated", "was_reset")
STATE = ("_cells", "agents", "rng", "step_count", "aux", "episode")
FIRST_ENV, K_POOL, T_STEPS = 11, 3, 10


def ar_state(spec, B, seed):
    """Random states with envs that restart at the first step -- step_count at max_steps - 1 (every 4th env), every agent terminated
    (the next one) -- and a pool of three fresh layouts"""
    st = util.random_state(spec, B, seed, density=0.3)
    b = np.arange(B)
    st["step_count"][b % 4 == 0] = spec.max_steps - 1
    st["agents"][b % 4 == 1, :, 4] = 1
    p = util.random_state(spec, K_POOL, seed + 1, density=0.3, terminated_p=0.0)
    return st, (p["grid"], p["agents"])


def pooled_env(spec, B, seed, device=DEV, specialise=True):
    st, pool = ar_state(spec, B, seed)
    kw = {} if torch.device(device).type == "cuda" else {"backend": util.OracleBackend(spec, nthreads=4)}
    env = BatchedMultiGridEnv(spec, B, device, first_env=FIRST_ENV, **kw)
    env.load_state(st["grid"], st["agents"], st["rng"], None, st["step_count"], validate=False)
    env.set_layout_pool(*pool)
    if specialise and not kw:
        assert env.specialise() in ("compiled", "registered")
        assert env.backend.launch_info(B)["fixed_shape"] == RUNTIME_COMPILED
    return env


def host_acts(spec, B, T, seed):
    return np.stack([util.random_actions(B, spec.num_agents, seed=seed + t) for t in range(T)])


def assert_equals_oracle(env, ref, ctx):
    for k in OUT + STATE:
        got, want = getattr(env, k).cpu().numpy(), getattr(ref, k).numpy()
        if got.tobytes() != want.tobytes():
            raise AssertionError(f"{ctx}: {k}: {es.first_difference(want, got)}")


# (spec, B): ragged batches -- no multiple of the 4 / 8 envs per wavefront --, the first of each a single wavefront
AR_CASES = [(SPEC_A, 3), (SPEC_A, 131), (SPEC_B, 5), (SPEC_B, 133)]


@pytest.mark.parametrize("spec,B", AR_CASES, ids=[f"{s.width}x{s.height}_a{s.num_agents}-B{B}" for s, B in AR_CASES])
def test_auto_reset_equals_the_oracle(spec, B):
    G = _lib.launch_info(spec, B)["envs_per_wavefront"]
    assert B % G != 0 and (B < G or B > 16 * G)              # ragged; a single wavefront, or many
    env, ref = pooled_env(spec, B, 40 + B), pooled_env(spec, B, 40 + B, "cpu")
    acts = host_acts(spec, B, T_STEPS, 300)
    resets = 0
    for t in range(T_STEPS):
        env.step(torch.from_numpy(acts[t]).to(DEV), auto_reset=True)
        ref.step(torch.from_numpy(acts[t]), auto_reset=True)
        assert_equals_oracle(env, ref, f"{spec.width}x{spec.height} B={B} step {t}")
        assert holds(env), f"step {t}: a marked env differs from its layout"
        resets += int(ref.was_reset.sum())
    assert env._bound[(True, False)][2], "step(auto_reset=True) did not go through mgx_step_tracked"
    assert resets >= B and int(ref.episode.min()) >= 1 and int((env._marker >= 0).sum()) > 0     # every env restarted; restarts mark
    env.check_errors()


@pytest.mark.parametrize("name", ["rbd_a3_all_v3", "lh12_a3_own_v7"])
def test_hooks_with_auto_reset_and_pool_aux(name):
    N = hs.BASE + 5
    env, rf = hk._ar_env(name, N), hk.ar_ref(name, True)
    assert env.specialise() in ("compiled", "registered")
    assert env.backend.launch_info(N)["fixed_shape"] == RUNTIME_COMPILED
    for t in range(hs.T_STEPS):
        outs = env.step(hk.script(name, N, t=t), auto_reset=True, hook_order=hk.script(name, N, "hook_order", t))
        rf.check_outputs(t, outs, f"{name} registered kernel, step {t}")
        rf.check_state(t, env, f"{name} registered kernel, step {t}", extra=("was_reset", "episode"))
        assert holds(env)
    env.check_errors()


@pytest.mark.parametrize("spec,B", [(SPEC_A, 131), (SPEC_B, 133)], ids=["7x6_a3", "6x5_a2"])
def test_under_capture(spec, B):
    env, ref = pooled_env(spec, B, 60 + B), pooled_env(spec, B, 60 + B, "cpu")
    T = 7
    acts = host_acts(spec, B, T, 400)
    graph = env.capture_steps(torch.from_numpy(acts).to(DEV), auto_reset=True, sub_shards=1)
    assert graph.sub_shards == 1 and graph._tracked
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for t in range(T):
            ref.step(torch.from_numpy(acts[t]), auto_reset=True)
        assert_equals_oracle(env, ref, f"{spec.width}x{spec.height} B={B} replay {replay}")
        assert holds(env)
    assert int(ref.episode.min()) >= 1
    env.check_errors()


@pytest.mark.parametrize("spec,B", [(SPEC_A, 131), (SPEC_B, 133)], ids=["7x6_a3", "6x5_a2"])
def test_with_episode_tracking(spec, B):
    env, ref = pooled_env(spec, B, 80 + B), pooled_env(spec, B, 80 + B, "cpu")
    stats = env.track_episodes()
    assert env.backend.launch_info(B)["fixed_shape"] == RUNTIME_COMPILED
    over0 = env.is_done().cpu().numpy()
    want = new_state(B, spec.num_agents)
    want["over"][:] = over0                                   # (an env that is over when tracking starts is skipped until it restarts)
    assert over0.sum() >= B // 4
    T = 2 * spec.max_steps + 3
    acts = host_acts(spec, B, T, 500)
    seen = {}
    for t in range(T):
        env.step(torch.from_numpy(acts[t]).to(DEV), auto_reset=True)
        ref.step(torch.from_numpy(acts[t]), auto_reset=True)
        assert_equals_oracle(env, ref, f"tracking, step {t}")
        model_stats(want, *record(env), BEFORE, seen=seen)
    assert_same_books(snapshot(stats), want, f"{spec.width}x{spec.height} B={B}")
    assert seen.get("trunc") and want["counts"][:, 0].min() >= 1 and not want["counts"][:, 3].any()
    env.check_errors()


def test_the_throughput_key_reads_the_marker():
    """ensure_shape(latency_only=False): a run-time compiled kernel WITHOUT the LDS-DMA tile loads -- hence with MARK_RD -- at the
    smallest batch of more than 2048 wavefronts.  (The code object has no scratch and no spills: tests/test_jit_shapes.py.)"""
    name = "8x8_a2_v5_jit"
    spec, B = ms.JIT_SIZES[name][0], ms.batch_of(name)
    key = jit.shape_key(spec, B)
    assert not key.dma and not key.built_in and ms.reads_marker(spec, B, 1)
    assert jit.ensure_shape(spec, B, DEV) in ("not-latency", "registered")
    assert jit.ensure_shape(spec, B, DEV, latency_only=False) in ("compiled", "registered")
    assert _lib.launch_info(spec, B)["fixed_shape"] == RUNTIME_COMPILED
    assert _lib.launch_info(spec, 4096)["fixed_shape"] == 0    # (the latency batches of the spec stay on the library's kernel)
    check_parity(name)
    run = ms.oracle_run(name)
    assert check_read(run.spec, run.B, run.pool)
    assert _lib.launch_info(spec, B)["fixed_shape"] == RUNTIME_COMPILED
