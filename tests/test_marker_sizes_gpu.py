"""The layout marker's READ (include/mgx.h: mgx_step_tracked; MARK_RD in csrc/mgx_fused_body.inc) at every grid size that qualifies,
and just outside.  tests/test_grid_layout_marker.py walks it at Empty-16x16 x 4 agents -- 512-byte grids, 16 envs per wavefront --
alone; grids of 32, 64, 128, 256 and 1024 bytes take the same path with other arithmetic: another number of envs per 1 KiB load
round, `lane16 & (HWB - 1)` the identity at 1 KiB, one agent (the rng loads "through a descriptor of no bytes"), a hook env with
`pool_aux`, a last wavefront with fewer envs than the others -- one env in two of the cases.  The cases, their batches (the smallest
of more than 2048 wavefronts plus a remainder) and the oracle's side are tests/marker_sizes.py.  Per size:

  * census, without a GPU: the ORACLE's run of the sampled wavefronts alone meets a wavefront whose envs are all marked at a step's
    start, one with marked and unmarked envs, a marked env that a pickup / toggle / drop dirties, an unmarked env that a restart
    marks.  All four apply to every size: the 4x4 grid, which random placement leaves no room on, is the Empty layout plus a key in
    front of the agent;
  * parity after every one of 12 steps (max_steps 4 or 5: every env restarts at least twice): the tracked env equals an untracked
    HIP twin over the whole batch, and the oracle on the sample -- outputs, state, aux, was_reset, episode, and the marker against
    its model; `holds`; no error word;
  * the read is really taken: cells overwritten behind the marker's back are NOT observed until the marker is taken back.
Just outside -- 32x32 (2 KiB), 8x6 (96 bytes: no power of two), 8x8 on two layouts, and 8x8 at 2048 wavefronts in either family -- the
overwritten cells are observed at once.  Every expectation of either kind is first held against `marker_sizes.reads_marker`, the
Python mirror of plan_marker_read's rule.

No spec reaches a power-of-two grid with a tile beyond 8 KiB: a wavefront's LDS budget of 12 KiB and its power-of-two env count cap
the tile of such grids at 8 KiB, so the `Gw * hwb <= 8192` clause has no case of its own."""
import numpy as np
import pytest
import torch

from multigrid_amd import EnvSpec, _lib
from tests import marker_sizes as ms
from tests import util
from tests.test_grid_layout_marker import DEV, assert_same, holds, make_env, untracked_stepper


@pytest.mark.parametrize("name", list(ms.CASES))
def test_the_oracle_alone_meets_the_census(name):
    run = ms.oracle_run(name)
    spec, B = run.spec, run.B
    assert ms.reads_marker(spec, B, 1) and ms.wavefronts(spec, B) == 2049 and ms.wavefronts(spec, B - ms.CASES[name][2]) == 2048
    (lo0, hi0), (lo1, hi1) = run.sample[0], run.sample[-1]
    assert lo0 == 0 and hi1 == B and 0 < hi1 - lo1 == ms.CASES[name][2] < hi0 - lo0        # the first wavefront, the partial last one
    for k in ms.CENSUS:
        assert run.census[k] > 0, f"{name}: {k} never happened in the oracle's run: {run.census}"
    assert sum(int(s["ambiguous"].sum()) for s in run.steps) <= 2, "the marker's model leaves too many envs open"


def test_batches_and_the_mirror_of_the_rule():
    lone = [n for n in ms.SIZES if ms.CASES[n][2] == 1]
    assert "4x4_a1_v3" in lone and "32x16_a2_v7" in lone
    assert sorted(s.width * s.height * 2 for s, _, _ in ms.SIZES.values()) == [32, 64, 128, 256, 256, 1024]
    spec16 = EnvSpec(16, 16, 4, 7, max_steps=8)
    assert ms.reads_marker(spec16, 32784, 1) and not ms.reads_marker(spec16, 32784, 4) and not ms.reads_marker(spec16, 256, 1)
    for name, (spec, B, K) in outside_cases().items():
        assert not ms.reads_marker(spec, B, K), name
    spec8 = ms.SIZES["8x8_a2_v7"][0]
    B = ms.smallest_reading_batch(spec8)
    assert ms.reads_marker(spec8, B, 1) and ms.wavefronts(spec8, B - 1) == 2048
    Bt = ms.throughput_batch_of_2048_wavefronts(spec8)
    assert Bt is not None and Bt > B and ms.wavefronts(spec8, Bt) == 2048 and ms.reads_marker(spec8, Bt + 1, 1)


# ---- parity ---------------------------------------------------------------------------------------------------------------------------

def check_parity(name, prepare=None):
    """Twelve tracked steps against the untracked twin (whole batch) and the oracle (the sampled wavefronts); prepare(env) runs on
    both HIP envs before the first step."""
    run = ms.oracle_run(name)
    spec, B, pool = run.spec, run.B, run.pool
    assert ms.reads_marker(spec, B, 1)
    e1, e2 = make_env(spec, B, pool), make_env(spec, B, pool)
    for e in (e1, e2):
        if prepare is not None:
            prepare(e)
    step2 = untracked_stepper(e2)
    acts = torch.from_numpy(run.acts).to(DEV)
    idx = torch.from_numpy(run.idx).to(DEV)
    assert int((e1._marker == 0).sum()) == B                  # armed by the comparison with the one layout
    drift = np.zeros(len(run.idx), bool)                      # sampled envs whose marker went -1 where the model could not tell
    for t in range(ms.T_STEPS):
        ctx = f"{name} B={B} step {t}"
        e1.step(acts[t], auto_reset=True)
        step2(acts[t])
        assert_same(e1, e2, ctx)
        assert holds(e1), f"{ctx}: a marked env differs from its layout"
        want = run.steps[t]
        for k in ms.OUT + ms.STATE:
            got = getattr(e1, k)[idx].cpu().numpy()
            if got.tobytes() != want[k].tobytes():
                bad = np.nonzero((got != want[k]).reshape(len(run.idx), -1).any(axis=1))[0]
                raise AssertionError(f"{ctx}: {k} differs from the oracle in env(s) {run.idx[bad][:8].tolist()} ({len(bad)} of the sample)")
        got = e1._marker[idx].cpu().numpy()
        drift &= want["was_reset"] == 0
        drift |= want["ambiguous"] & (got == -1)
        model = np.where(drift, -1, want["_marker"])
        bad = np.nonzero(got != model)[0]
        assert len(bad) == 0, f"{ctx}: the marker of env(s) {run.idx[bad][:8].tolist()} is {got[bad][:8].tolist()}, the model says {model[bad][:8].tolist()}"
    assert e1._bound[(True, False)][2], "step(auto_reset=True) did not go through mgx_step_tracked"
    assert int(e1.episode.min()) >= 2                          # every env restarted at least twice
    assert int((e1._marker < 0).sum()) > 0 and int((e1._marker >= 0).sum()) > 0
    e1.check_errors()
    e2.check_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ms.SIZES))
def test_tracked_steps_equal_the_untracked_twin_and_the_oracle(name):
    check_parity(name)
    spec, B = ms.SIZES[name][0], ms.batch_of(name)
    assert _lib.launch_info(spec, B)["fixed_shape"] == 0      # the library's generic kernel


# ---- the read is taken, or not ----------------------------------------------------------------------------------------------------------

def tricked_envs(spec, B, pool, prepare=None):
    """(an env on its layouts, one whose cells were overwritten behind the marker's back, one that holds the overwritten cells the
    regular way), every env marked with its layout in the first two and unknown in the third; nobody restarts within two steps"""
    K = pool[0].shape[0]
    others = np.stack([ms.visible_change(spec, tuple(None if p is None else p[k:k + 1] for p in pool))[0] for k in range(K)])
    true_env, tricked = make_env(spec, B, pool), make_env(spec, B, pool)
    over = make_env(spec, B, (others,) + tuple(pool[1:]))
    over.set_layout_pool(*pool)                                # (the same shapes: refilled in place, compared again)
    for e in (true_env, tricked, over):
        if prepare is not None:
            prepare(e)
        e.step_count.zero_()
    if K > 1:                                                  # several layouts: nothing is compared; the promise is true all the same
        for e in (true_env, tricked):
            e._marker.copy_(torch.arange(B, device=DEV) % K)
            e._mark["armed"] = True
    want = (torch.arange(B, device=DEV) % K).to(torch.int32)
    assert torch.equal(tricked._marker, want) and torch.equal(true_env._marker, want) and int((over._marker >= 0).sum()) == 0
    assert holds(tricked) and not torch.equal(over._cells, tricked._cells)
    tricked._cells.copy_(over._cells)                          # behind the marker's back
    return true_env, tricked, over


def check_read(spec, B, pool, prepare=None):
    """What the step of a wavefront observes whose envs are all marked while their cells say something else: the layout where the
    launch reads the marker (and the cells once the marker is taken back), the cells at once where it does not."""
    reads = ms.reads_marker(spec, B, pool[0].shape[0])
    true_env, tricked, over = tricked_envs(spec, B, pool, prepare)
    noop = torch.full((B, spec.num_agents), ms.DONE, dtype=torch.int8, device=DEV)      # `done`: nobody moves, nothing is written
    for e in (true_env, tricked, over):
        e.step(noop, auto_reset=True)
        assert e._bound[(True, False)][2]
    assert not torch.equal(true_env.obs, over.obs)
    if reads:
        assert torch.equal(tricked.obs, true_env.obs), "a launch that should read the marker observed the cells in device memory"
        tricked._marker.fill_(-1)
        for e in (tricked, over):
            e.step(noop, auto_reset=True)
    else:
        same = (tricked.obs == true_env.obs).flatten(1).all(dim=1)
        assert not bool(same.any()), f"{int(same.sum())} env(s) of a launch that should not read the marker observed the pool's layout"
    assert torch.equal(tricked.obs, over.obs)
    for e in (true_env, tricked, over):
        e.check_errors()
    return reads


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ms.SIZES))
def test_a_marked_wavefront_reads_the_pool_not_its_grids(name):
    run = ms.oracle_run(name)
    assert check_read(run.spec, run.B, run.pool)


OUTSIDE = ("32x32_2048_bytes", "8x6_96_bytes", "8x8_2048_wavefronts_latency_family", "8x8_2048_wavefronts_throughput_family",
           "8x8_two_layouts")


def outside_cases():
    """name -> (spec, batch, layouts in the pool)"""
    spec8 = ms.SIZES["8x8_a2_v7"][0]
    B8 = ms.smallest_reading_batch(spec8)
    big, odd = EnvSpec(32, 32, 2, 7, max_steps=5), EnvSpec(8, 6, 2, 7, max_steps=5)
    return {"32x32_2048_bytes": (big, ms.smallest_reading_batch(big) + 2, 1),
            "8x6_96_bytes": (odd, ms.smallest_reading_batch(odd) + 2, 1),
            "8x8_2048_wavefronts_latency_family": (spec8, B8 - 1, 1),
            # (the batch before the smallest reading one is stepped by the latency family, which never reads; this one has 2048
            # wavefronts of the THROUGHPUT family -- 64 view slots each --: the launch at which `> 2048` is the whole difference)
            "8x8_2048_wavefronts_throughput_family": (spec8, ms.throughput_batch_of_2048_wavefronts(spec8), 1),
            "8x8_two_layouts": (spec8, B8 + 4, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", OUTSIDE)
def test_just_outside_the_cells_are_observed_at_once(name):
    assert tuple(outside_cases()) == OUTSIDE
    spec, B, K = outside_cases()[name]
    if K == 1:
        pool = ms.pool_for(spec, 6)
    else:
        st = util.random_state(spec, K, 6, density=0.3, terminated_p=0.0)
        pool = (st["grid"], st["agents"], None)
    assert ms.wavefronts(spec, B) >= 2048
    assert not check_read(spec, B, pool)
