"""The producer kernels of the persistent hand-shake -- persistent_post_kernel, persistent_wait_kernel, persistent_feed_kernel<4|2|1|0>
(csrc/mgx_aux.hip) -- path by path against the NumPy model of tests/persist_cases.py, and the consumer's wait for a step's granules
that arrive in two parts.

No standing session is needed for the producers: the post is a map from actions to granules, the wait reads a flag array, and the feed
runs to its end without a resident launch when done[] already holds the last step's number -- it then leaves the granules of step T
behind.  Every comparison is exact (on the tag and on the bytes of agents < A: include/mgx.h leaves the others open).  The C ABI is
called directly (ctypes) so that pointers can be offset; every buffer sits between guard bytes that must come back unchanged.  Which
kernel paths the cases reach is derived and asserted on the CPU by tests/test_persist_branch_census.py.  Every outcome is decided by
constant data, never by timing: a wait either finds all of its flags there, or one flag stays behind for good and the wait's
documented bounded return (1 ms) is what is checked."""
import ctypes as C

import numpy as np
import pytest
import torch

from multigrid_amd import EnvSpec, _lib
from multigrid_amd.batched import BatchedMultiGridEnv
from tests import persist_cases as pc
from tests import util
from tests.test_aux_kernels_gpu import DEV, Buf, stream

gpu = pytest.mark.gpu
U32_MAX = 2 ** 32 - 1
CTRL0 = np.array([0, 0, 0, U32_MAX, 0, 0, 0, 0], np.uint32)        # include/mgx.h: zeroed by the caller except [3]


def c_spec(A):
    return EnvSpec(16, 16, A, 3).to_c()


def sync():
    torch.cuda.current_stream().synchronize()


def assert_granules(got, actions, tag, ctx):
    """got u64[B * gpe] == the model on the tag and on the bytes of agents < A"""
    A = actions.shape[1]
    want, mask = pc.granules_reference(actions, tag), pc.granule_mask(A)
    got = got.reshape(want.shape)
    bad = (got & mask) != (want & mask)
    if bad.any():
        b, q = (int(v[0]) for v in np.nonzero(bad))
        pytest.fail(f"{ctx}: {int(bad.sum())} of {bad.size} granules differ; the first is granule {q} of env {b} (granule "
                    f"{b * want.shape[1] + q} in all): got {int(got[b, q]):#018x}, want {int(want[b, q]):#018x} under mask "
                    f"{int(mask[q]):#018x}; the env's actions {actions[b].tolist()}")


# ===================================================================================================================== post
@gpu
@pytest.mark.parametrize("case", pc.POST, ids=pc.POST_IDS)
def test_post_every_granule_tag_and_guard(case):
    L = _lib.lib()
    A, B = case.A, case.B
    act1, act2 = pc.post_inputs(case)
    ng = B * pc.gpe_of(A)
    d_act, d_gr = Buf(B * A, case.act_off, act1), Buf(ng * 8, case.gr_off)
    sc = c_spec(A)
    assert L.mgx_persistent_post(C.byref(sc), B, d_act.ptr, case.tag, d_gr.ptr, stream()) == 0
    assert_granules(d_gr.get(np.uint64), act1, case.tag, "first post")
    np.testing.assert_array_equal(d_act.get(np.int8).reshape(B, A), act1)
    assert d_gr.guards_intact() and d_act.guards_intact()
    # another step's actions under another tag into the same buffer: every granule is replaced
    tag2 = case.tag ^ 0x80000003
    d_act2 = Buf(B * A, case.act_off, act2)
    assert L.mgx_persistent_post(C.byref(sc), B, d_act2.ptr, tag2, d_gr.ptr, stream()) == 0
    assert_granules(d_gr.get(np.uint64), act2, tag2, "second post")
    assert d_gr.guards_intact() and d_act2.guards_intact()


# ===================================================================================================================== wait
def run_wait(L, flags, waves, step, d_ctrl, timeout_ms):
    """flags u32[waves]; behind them WAIT_TAIL zero words, then the guard.  Returns ctrl after the wait."""
    words = np.concatenate([flags.astype(np.uint32), np.zeros(pc.WAIT_TAIL, np.uint32)])
    d_done = Buf(words.nbytes, data=words)
    assert L.mgx_persistent_wait(d_done.ptr, waves, step, d_ctrl.ptr, timeout_ms, stream()) == 0
    sync()
    np.testing.assert_array_equal(d_done.get(np.uint32), words)
    assert d_done.guards_intact() and d_ctrl.guards_intact()
    return d_ctrl.get(np.uint32)


@gpu
@pytest.mark.parametrize("waves", pc.WAIT_WAVES)
@pytest.mark.parametrize("mixed", [False, True], ids=["all_equal", "mixed"])
def test_wait_returns_at_once_when_every_flag_is_there(waves, mixed):
    """... whatever lies behind done[waves): 64 zero words, which no step >= 1 is satisfied by"""
    L = _lib.lib()
    step = 7
    flags = np.full(waves, step, np.uint32)
    if mixed:
        r = pc._rng("wait mixed", waves)
        later = r.choice(np.array([step + 1, 2 ** 31 - 1, 2 ** 31, U32_MAX], np.uint32), size=waves)
        flags = np.where(r.random(waves) < 0.5, flags, later).astype(np.uint32)
        flags[-1] = U32_MAX
    d_ctrl = Buf(32, data=CTRL0)
    ctrl = run_wait(L, flags, waves, step, d_ctrl, 2000)
    assert ctrl[1] == 0 and ctrl[4] == 0
    np.testing.assert_array_equal(ctrl, CTRL0)


@gpu
@pytest.mark.parametrize("waves", pc.WAIT_WAVES)
def test_wait_sees_one_late_flag_wherever_it_sits(waves):
    """One flag stays at step - 1 for good: the wait's bounded return (1 ms) reports it, for every position the late flag can take
    relative to the 256 threads and the pass of 2048.  ctrl[4] is sticky (include/mgx.h): a wait on the same ctrl whose flags are all
    there reports a timeout too."""
    L = _lib.lib()
    step = 1000
    for pos in pc.wait_late_positions(waves):
        flags = np.full(waves, step, np.uint32)
        flags[pos] = step - 1
        d_ctrl = Buf(32, data=CTRL0)
        ctrl = run_wait(L, flags, waves, step, d_ctrl, 1)
        assert ctrl[1] == 1 and ctrl[4] == 1, f"late flag at {pos} of {waves}: ctrl {ctrl.tolist()}"
        assert ctrl[[0, 2, 3, 5, 6, 7]].tolist() == CTRL0[[0, 2, 3, 5, 6, 7]].tolist()
        ctrl = run_wait(L, np.full(waves, step, np.uint32), waves, step, d_ctrl, 2000)
        assert ctrl[1] == 2 and ctrl[4] == 1, f"after the late flag at {pos} of {waves}: ctrl {ctrl.tolist()}"


# ===================================================================================================================== feed
def run_feed(L, A, B, T, actions, act_off, waves, done_value, timeout_ms, trace):
    """mgx_persistent_feed on its own.  Returns (granules u64, ctrl u32[8], trace u64[2T + 1] or None)."""
    ng = B * pc.gpe_of(A)
    d_act, d_gr = Buf(actions.nbytes, act_off, actions), Buf(ng * 8)
    d_done, d_ctrl = Buf(waves * 4, data=np.full(waves, done_value, np.uint32)), Buf(32, data=CTRL0)
    d_tr = Buf((2 * T + 1) * 8, data=np.zeros(2 * T + 1, np.uint64)) if trace else None
    pers = _lib.MgxPersistent(d_gr.ptr, d_done.ptr, d_ctrl.ptr, T, timeout_ms)
    sc = c_spec(A)
    rc = L.mgx_persistent_feed(C.byref(sc), B, d_act.ptr, T, C.byref(pers), waves, d_tr.ptr if trace else None, stream())
    assert rc == 0
    sync()
    for d in (d_act, d_gr, d_done, d_ctrl) + ((d_tr,) if trace else ()):
        assert d.guards_intact()
    np.testing.assert_array_equal(d_act.get(np.int8), actions.reshape(-1))
    assert (d_done.get(np.uint32) == done_value).all()
    return d_gr.get(np.uint64), d_ctrl.get(np.uint32), d_tr.get(np.uint64) if trace else None


@gpu
@pytest.mark.parametrize("first_only", [False, True], ids=["T", "T1"])
@pytest.mark.parametrize("case", pc.FEED, ids=pc.FEED_IDS)
def test_feed_alone_leaves_the_last_steps_granules(case, first_only):
    """done[] = T throughout: every wait of the kernel is satisfied by constant data, and what is left behind are the granules of
    step T.  At T = 1 these come from the fetch ahead of the loop alone."""
    L = _lib.lib()
    A, B = case.A, case.B
    T = 1 if first_only else case.T
    actions = pc.feed_inputs(case)[:T].copy()
    got, ctrl, tr = run_feed(L, A, B, T, actions, case.act_off, case.waves, T, 2000, case.trace)
    assert_granules(got, actions[T - 1], T, f"step {T}")
    assert ctrl[0] == 0 and ctrl[1] == 0 and ctrl[4] == 0, ctrl.tolist()
    np.testing.assert_array_equal(ctrl, CTRL0)
    if case.trace:
        assert tr[0] > 0 and (np.diff(tr.astype(np.int64)) >= 0).all(), tr.tolist()


_outlived = {}


def outlived():
    """the one run the two tests below look at: (actions, granules, ctrl, trace)"""
    if not _outlived:
        o = pc.OUTLIVE
        actions = pc.random_actions(pc._rng("outlive"), (o["T"], o["B"], o["A"]))
        _outlived["run"] = (actions,) + run_feed(_lib.lib(), o["A"], o["B"], o["T"], actions, 0, o["waves"], o["done"], 1, True)
    return _outlived["run"]


@gpu
def test_feed_that_outlives_its_consumer_stops_where_the_flags_stop():
    """done[] stays at 2 of T = 5: steps 1 .. 3 are posted (step 3 behind the outputs of step 2), the wait for step 3's outputs runs
    into the 1 ms timeout; the granules are step 3's in every workgroup's slice, the kernel counts one timeout and asks the launch
    to stop."""
    actions, got, ctrl, tr = outlived()
    posted = pc.OUTLIVE["done"] + 1
    assert_granules(got, actions[posted - 1], posted, "the last step posted")
    assert ctrl[0] == 1 and ctrl[1] == 1, ctrl.tolist()
    assert ctrl[4] == 1 and ctrl[[2, 3, 5, 6, 7]].tolist() == CTRL0[[2, 3, 5, 6, 7]].tolist()


@gpu
def test_feed_that_outlives_its_consumer_leaves_the_trace_zero_from_word_5_on():
    """The same run's trace: nothing from the stamp of the post nobody saw complete on.  include/mgx.h: a post's word is stored
    together with the word that follows it, so after three posts of which the third never completed words 0 .. 4 are written --
    seen, posted, seen, posted, seen -- and word 5 = [2 * (3 - 1) + 1] and everything behind it are as the caller left them.

    (The kernel used to store word 5 right behind the third post -- measured on an MI355X: [59024793925536, 59024793925600,
    59024793925700, 59024793925756, 59024793925816, 59024793925872, 0, 0, 0, 0, 0] --, a stamp for a step whose hand-shake was
    never finished; this test found it.)"""
    tr = outlived()[3]
    print("trace:", tr.tolist())
    assert (tr[5:] == 0).all(), tr.tolist()
    assert (tr[:5] > 0).all() and (np.diff(tr[:5].astype(np.int64)) >= 0).all(), tr.tolist()


# ===================================================================================================================== consumer
@gpu
@pytest.mark.parametrize("name,kw,B", pc.TWO_PART, ids=[c[0] for c in pc.TWO_PART])
def test_a_wavefront_waits_for_the_second_part_of_its_granules(name, kw, B):
    """Each step's granules arrive in two posts, cut inside wavefront k's envs.  Between the posts the wavefronts below k publish
    their flags (awaited: that is the kernel's own wait on done[0:k]); wavefront k, which has one env's granules, and every one
    above it must not have published -- a wavefront that lacks a granule can never have stepped.  After the second post the step
    completes and equals mgx_step's, output by output."""
    L = _lib.lib()
    spec = EnvSpec(**kw)
    A, T = spec.num_agents, pc.TWO_PART_STEPS
    st = util.random_state(spec, B, seed=len(name))
    e_ref, e_per = BatchedMultiGridEnv(spec, B, DEV), BatchedMultiGridEnv(spec, B, DEV)
    for e in (e_ref, e_per):
        e.load_state(st["grid"], st["agents"], st["rng"], st["target"], st["step_count"])
    G = _lib.launch_info(spec, B, persistent=True)["envs_per_wavefront"]
    acts = torch.from_numpy(np.stack([util.random_actions(B, A, seed=300 + t) for t in range(T)])).to(DEV)
    sc, gpe = spec.to_c(), pc.gpe_of(A)
    with e_per.persistent(max_steps=T) as ps:
        k = ps.waves // 2
        lo = k * G + 1
        assert ps.waves == -(-B // G) and 1 <= k and lo < min((k + 1) * G, B), (ps.waves, G)
        d_ctrl = Buf(32, data=CTRL0)                                      # (the partial waits' own ctrl: the session's stays clean)
        for t in range(1, T + 1):
            a = acts[t - 1]
            want = [x.clone() for x in e_ref.step(a)]
            assert L.mgx_persistent_post(C.byref(sc), lo, a.data_ptr(), t, ps.granules.data_ptr(), stream()) == 0
            assert L.mgx_persistent_wait(ps.done.data_ptr(), k, t, d_ctrl.ptr, 2000, stream()) == 0
            done = ps.done.cpu().numpy().view(np.uint32)
            c = d_ctrl.get(np.uint32)
            assert c[1] == 0 and c[4] == 0, f"step {t}: the wavefronts below {k} did not publish"
            assert (done[:k] == t).all()
            assert (done[k:] == t - 1).all(), f"step {t}: wavefronts {(np.nonzero(done[k:] != t - 1)[0] + k).tolist()} published " \
                                              f"without all of their granules"
            assert L.mgx_persistent_post(C.byref(sc), B - lo, a.data_ptr() + lo * A, t, ps.granules.data_ptr() + lo * gpe * 8,
                                         stream()) == 0
            ps.t = t                                                      # (posted by hand: the session's wait is for step t)
            got = ps.wait()
            for n, w, g in zip(("obs", "dir", "reward", "terminated", "truncated"), want, got):
                assert torch.equal(w, g), f"{name} step {t}: {n}"
    assert ps.timeouts == 0 and ps.steps_completed == T
    for n in ("cells", "agents", "rng", "step_count"):
        assert torch.equal(getattr(e_ref, n), getattr(e_per, n)), f"{name}: {n} after the session"
    assert d_ctrl.guards_intact()
