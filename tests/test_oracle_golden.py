"""Pin the CPU oracle (oracle/mgx_oracle.c) against vectors produced by the real reference.

The fixtures in tests/golden/ were written by oracle/gen_golden.py running ini/multigrid itself in the build
container.  Bit-exact on everything: obs images, direction, rewards (float64 equality), terminations,
truncations, post-step grid/agent state, visiting order and the PCG64 stream.
"""
import glob
import json
import os

import numpy as np
import pytest

from oracle import binding as ob

GOLDEN = [p for p in sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
          if not os.path.basename(p).startswith(("layout_", "wrappers_", "custom_", "customsteps_", "randstate_", "resets_", "conflict_"))]


def load(path):
    z = np.load(path)
    spec = json.loads(str(z["spec_json"]))
    return z, spec


def rng_lohi(words_hilo):
    hi_s, lo_s, hi_i, lo_i = (int(w) for w in words_hilo)
    return np.array([lo_s, hi_s, lo_i, hi_i], dtype=np.uint64)


def test_fixtures_present():
    assert len(GOLDEN) >= 20


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_oracle_replays_reference(path):
    z, spec = load(path)
    from tests import util
    env = ob.RefEnv(spec, z["grid0"], z["agents0"], rng_lohi(z["rng0"]), target=[int(v) for v in util.golden_aux(spec)])
    np.testing.assert_array_equal(env.gen_obs(), z["obs0"].astype(np.int64))
    T = z["actions"].shape[0]
    for t in range(T):
        # (*_dictorder fixtures: the reference was stepped with a dict whose keys were inserted in this order)
        obs, direction, reward, terminated, truncated, order = env.step(
            z["actions"][t], hook_order=z["hook_order"][t] if "hook_order" in z.files else None)
        ctx = f"{os.path.basename(path)} step {t}"
        np.testing.assert_array_equal(order, z["order"][t], err_msg=ctx)
        np.testing.assert_array_equal(obs, z["obs"][t].astype(np.int64), err_msg=ctx)
        np.testing.assert_array_equal(direction, z["direction"][t], err_msg=ctx)
        assert reward.tobytes() == z["reward"][t].tobytes(), ctx          # float64 bit equality
        np.testing.assert_array_equal(terminated, z["terminated"][t].astype(bool), err_msg=ctx)
        assert truncated == bool(z["truncated"][t]), ctx
        np.testing.assert_array_equal(env.grid_state, z["grid"][t].astype(np.int64), err_msg=ctx)
        np.testing.assert_array_equal(env.agent_state, z["agents"][t].astype(np.int64), err_msg=ctx)
    np.testing.assert_array_equal(env.rng, rng_lohi(z["rng_final"]))


def test_dict_order_fixtures_pin_the_hook_visiting_order():
    """The *_dictorder fixtures must be cases where the visiting order of the env hooks (the caller's dict order,
    redbluedoors.py:176 / locked_hallway.py:210) changes the result: replayed with ascending order the oracle must DIFFER."""
    from tests import util
    differs = 0
    for path in GOLDEN:
        if "_dictorder_" not in path:
            continue
        z, spec = load(path)
        env = ob.RefEnv(spec, z["grid0"], z["agents0"], rng_lohi(z["rng0"]), target=[int(v) for v in util.golden_aux(spec)])
        for t in range(z["actions"].shape[0]):
            _, _, reward, terminated, _, _ = env.step(z["actions"][t])          # ascending
            if reward.tobytes() != z["reward"][t].tobytes() or not np.array_equal(terminated, z["terminated"][t].astype(bool)):
                differs += 1
                break
    assert differs >= 2


def test_goldens_cover_the_dynamics():
    """The fixture set must actually exercise pickup, drop, door open/close/unlock, box toggle, success,
    failure, truncation and an unseen-masked cell -- otherwise the pin is hollow."""
    seen = dict(pickup=0, drop=0, door_open=0, door_close=0, unlock=0, box_gone=0, success=0, lava=0,
                trunc=0, unseen=0, agent_seen=0)
    for path in GOLDEN:
        z, spec = load(path)
        agents = np.concatenate([z["agents0"][None].astype(np.int64), z["agents"].astype(np.int64)])
        grid = np.concatenate([z["grid0"][None].astype(np.int64), z["grid"].astype(np.int64)])
        carry = agents[:, :, 6]
        seen["pickup"] += int(((carry[:-1] == 1) & (carry[1:] != 1)).sum())
        seen["drop"] += int(((carry[:-1] != 1) & (carry[1:] == 1)).sum())
        door = (grid[:-1, ..., 0] == 4) & (grid[1:, ..., 0] == 4)
        s0, s1 = grid[:-1, ..., 2], grid[1:, ..., 2]
        seen["door_open"] += int((door & (s0 == 1) & (s1 == 0)).sum())
        seen["door_close"] += int((door & (s0 == 0) & (s1 == 1)).sum())
        seen["unlock"] += int((door & (s0 == 2) & (s1 == 0)).sum())
        box_cells = (grid[:-1, ..., 0] == 7) & (grid[1:, ..., 0] == 1)
        picked = ((carry[:-1] == 1) & (carry[1:] == 7)).sum(axis=1)
        seen["box_gone"] += int((box_cells.sum(axis=(1, 2)) - picked > 0).sum())
        seen["success"] += int((z["reward"] > 0).any(axis=1).sum())
        seen["lava"] += int(((z["terminated"].sum(axis=1) > 0) & ~(z["reward"] > 0).any(axis=1)).any())
        seen["trunc"] += int(z["truncated"].any())
        seen["unseen"] += int((z["obs"][..., 0] == 0).any())
        seen["agent_seen"] += int((z["obs"][..., 0] == 10).any())
    missing = [k for k, v in seen.items() if v == 0]
    assert not missing, (missing, seen)


@pytest.mark.parametrize("seed", [0, 7, 123, 2**40 + 5])
def test_pcg64_matches_numpy(seed):
    bg = np.random.PCG64(np.random.SeedSequence(seed))
    st = bg.state["state"]
    m = (1 << 64) - 1
    words = np.array([st["state"] & m, st["state"] >> 64, st["inc"] & m, st["inc"] >> 64], dtype=np.uint64)
    want = np.random.Generator(bg).random(64)
    got = ob.pcg64_random(words, 64)
    assert got.tobytes() == want.tobytes()
    st2 = bg.state["state"]
    assert int(words[0]) | (int(words[1]) << 64) == st2["state"]


def test_unknown_action_raises_value_error():
    path = [p for p in GOLDEN if "empty8_a2_seed0" in p][0]
    z, spec = load(path)
    env = ob.RefEnv(spec, z["grid0"], z["agents0"], rng_lohi(z["rng0"]))
    with pytest.raises(ValueError):
        env.step(np.array([7, 0], dtype=np.int8))


def test_oracle_wrappers_match_reference():
    """OneHotObsWrapper / FullyObsWrapper restatements vs outputs of the real reference wrappers."""
    from tests import util
    assert util.WRAPPER_GOLDEN
    for path in util.WRAPPER_GOLDEN:
        z = np.load(path)
        for t in range(z["obs"].shape[0]):
            np.testing.assert_array_equal(ob.one_hot(z["obs"][t]), z["one_hot"][t])
            np.testing.assert_array_equal(ob.full_obs(z["grid"][t], z["agents"][t]), z["full"][t].astype(np.int64))


PY_GOLDEN = [p for p in GOLDEN if os.path.basename(p).startswith(("empty8_a2_seed0", "empty16_a4_seed1", "empty16_a4_objects", "empty8_a2_unlock",
                                                                  "bup_a2_seed", "emptyrandom6_a3_nooverlap"))]


@pytest.mark.parametrize("path", PY_GOLDEN, ids=[os.path.basename(p)[:-4] for p in PY_GOLDEN])
def test_python_restatement_replays_reference(path):
    """oracle/py_oracle.py -- the pure Python / NumPy per-env restatement bench.py times on one host core as the reference's
    interpreter-speed stand-in -- against what the real reference produced: every output, every step."""
    from oracle import py_oracle as po
    z, spec = load(path)
    assert PY_GOLDEN
    grid, agents = z["grid0"].astype(np.int64), z["agents0"].astype(np.int64)
    hs, ls, hi, li = (int(w) for w in z["rng0"])
    bg = np.random.PCG64()
    st = bg.state
    st["state"] = {"state": (hs << 64) | ls, "inc": (hi << 64) | li}
    st["has_uint32"], st["uinteger"] = 0, 0
    bg.state = st
    rng = np.random.Generator(bg)
    np.testing.assert_array_equal(po.gen_obs(grid, agents, spec["view_size"], spec["see_through_walls"]), z["obs0"])
    sc = 0
    T = min(z["actions"].shape[0], 120)
    for t in range(T):
        obs, d, rew, term, trunc, sc = po.step(spec, grid, agents, rng, sc, z["actions"][t], spec.get("target"))
        ctx = f"step {t}"
        np.testing.assert_array_equal(obs, z["obs"][t], err_msg=ctx)
        np.testing.assert_array_equal(d, z["direction"][t], err_msg=ctx)
        assert rew.tobytes() == z["reward"][t].tobytes(), ctx
        np.testing.assert_array_equal(term.astype(np.uint8), z["terminated"][t], err_msg=ctx)
        assert bool(trunc) == bool(z["truncated"][t]), ctx
        np.testing.assert_array_equal(grid, z["grid"][t].astype(np.int64), err_msg=ctx)
        np.testing.assert_array_equal(agents, z["agents"][t].astype(np.int64), err_msg=ctx)


# ---------------------------------------------------------------------------------------------------------- random-state corpus
# tests/golden/randstate_*.npz (oracle/gen_golden.py: record_random_states): batches of tests.util.random_state envs -- the states the
# GPU suite runs on -- loaded into the REAL reference and stepped there.  Product layout, batch-major per step.

def _randstate(path):
    from tests import util
    z, d, spec = util.load_golden(path)
    return z, d, spec


@pytest.mark.parametrize("path", __import__("tests.util", fromlist=["RANDSTATE_GOLDEN"]).RANDSTATE_GOLDEN,
                         ids=__import__("tests.util", fromlist=["RANDSTATE_IDS"]).RANDSTATE_IDS)
def test_oracle_replays_reference_random_states(path):
    """ob.step_batch on the whole batch against the reference's own bytes: every output, the post-step grid, agents, generator
    words and step count, every step."""
    z, d, spec = _randstate(path)
    sd = spec.as_dict()
    grid, agents = z["grid0"].copy(), z["agents0"].copy()
    rng, sc = z["rng0"].copy(), z["step_count0"].copy()
    aux = z["aux"].copy() if spec.env_kind != "empty" else None
    o, dr = ob.gen_obs_batch(sd, grid, agents)
    np.testing.assert_array_equal(o, z["obs0"])
    np.testing.assert_array_equal(dr, z["dir0"])
    for t in range(z["actions"].shape[0]):
        o, dr, rw, te, tr = ob.step_batch(sd, grid, agents, rng, sc, np.ascontiguousarray(z["actions"][t]), aux)
        ctx = f"{os.path.basename(path)} step {t}"
        np.testing.assert_array_equal(o, z["obs"][t], err_msg=ctx)
        np.testing.assert_array_equal(dr, z["dir"][t], err_msg=ctx)
        assert rw.tobytes() == z["reward"][t].tobytes(), ctx
        np.testing.assert_array_equal(te, z["terminated"][t], err_msg=ctx)
        np.testing.assert_array_equal(tr, z["truncated"][t], err_msg=ctx)
        np.testing.assert_array_equal(grid, z["grid"][t], err_msg=ctx)
        np.testing.assert_array_equal(agents, z["agents"][t], err_msg=ctx)
        np.testing.assert_array_equal(rng, z["rng"][t], err_msg=ctx)
        np.testing.assert_array_equal(sc, z["step_count0"] + t + 1, err_msg=ctx)


@pytest.mark.parametrize("path", __import__("tests.util", fromlist=["CONFLICT_GOLDEN"]).CONFLICT_GOLDEN,
                         ids=__import__("tests.util", fromlist=["CONFLICT_IDS"]).CONFLICT_IDS)
def test_oracle_replays_reference_conflicts(path):
    """The same on the constructed conflict corpus (tests/golden/conflict_*.npz, oracle/gen_golden.py: record_conflicts): the oracle
    is what the GPU suite compares with where the reference has nothing to record (unknown actions in a contended env)."""
    test_oracle_replays_reference_random_states(path)


def _filled_boxes(z):
    return bool(((z["grid0"][..., 0] == 7) & (z["grid0"][..., 2] >> 2 != 0)).any()
                or ((z["agents0"][..., 5] == 7) & (z["agents0"][..., 7] >> 2 != 0)).any())


def _py_randstate():
    from tests import util
    return [p for p in util.RANDSTATE_GOLDEN if not _filled_boxes(np.load(p))]


def test_py_restatement_leaves_out_only_the_filled_box_fixtures():
    """oracle/py_oracle.py has no box contents (its docstring): the fixtures with filled boxes are the only ones it does not replay."""
    from tests import util
    left = sorted(set(util.RANDSTATE_GOLDEN) - set(_py_randstate()))
    assert [os.path.basename(p) for p in left] == ["randstate_10x9_a3_v7_boxes.npz"], left


@pytest.mark.parametrize("path", _py_randstate(), ids=lambda p: os.path.basename(p)[:-4])
def test_python_restatement_replays_reference_random_states(path):
    """oracle/py_oracle.py, env by env, in the reference's own array shapes, against the reference's bytes."""
    from multigrid_amd import layouts
    from oracle import py_oracle as po
    z, d, spec = _randstate(path)
    B, T = z["grid0"].shape[0], z["actions"].shape[0]
    for b in range(B):
        grid = layouts.grid_from_product(z["grid0"][b])
        agents = layouts.unpack_agents(z["agents0"][b])
        ls, hs, li, hi = (int(w) for w in z["rng0"][b])
        bg = np.random.PCG64()
        st = bg.state
        st["state"] = {"state": (hs << 64) | ls, "inc": (hi << 64) | li}
        st["has_uint32"], st["uinteger"] = 0, 0
        bg.state = st
        rng = np.random.Generator(bg)
        sc = int(z["step_count0"][b])
        target = [int(v) for v in z["aux"][b, :3]]
        np.testing.assert_array_equal(po.gen_obs(grid, agents, spec.view_size, spec.see_through_walls), z["obs0"][b])
        for t in range(T):
            obs, dr, rew, term, trunc, sc = po.step(d, grid, agents, rng, sc, z["actions"][t, b], target)
            ctx = f"env {b} step {t}"
            np.testing.assert_array_equal(obs, z["obs"][t, b], err_msg=ctx)
            np.testing.assert_array_equal(dr, z["dir"][t, b], err_msg=ctx)
            assert rew.tobytes() == z["reward"][t, b].tobytes(), ctx
            np.testing.assert_array_equal(term.astype(np.uint8), z["terminated"][t, b], err_msg=ctx)
            assert int(trunc) == int(z["truncated"][t, b]), ctx
            np.testing.assert_array_equal(layouts.grid_to_product(grid), z["grid"][t, b], err_msg=ctx)
            np.testing.assert_array_equal(layouts.pack_agents(agents), z["agents"][t, b], err_msg=ctx)
            st = bg.state["state"]
            m = (1 << 64) - 1
            assert [st["state"] & m, st["state"] >> 64, st["inc"] & m, st["inc"] >> 64] == [int(w) for w in z["rng"][t, b]], ctx


def randstate_events(z, spec):
    """Counts of the events the random-state corpus must hold for its pin to mean anything (test_randstate_corpus_covers_...)."""
    grid = np.concatenate([z["grid0"][None], z["grid"]]).astype(np.int64)          # [T+1,B,H,W,3]
    ag = np.concatenate([z["agents0"][None], z["agents"]]).astype(np.int64)        # [T+1,B,A,8]
    act, rew, term, trunc = z["actions"].astype(np.int64), z["reward"], z["terminated"], z["truncated"].astype(bool)
    T, B, A = act.shape
    H, W = grid.shape[2:4]
    ev = {}
    g0, g1, a0, a1 = grid[:-1], grid[1:], ag[:-1], ag[1:]
    pos0 = a0[..., 2:4]                                                            # [T,B,A,2] (x, y)
    dvec = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)])
    front = pos0 + dvec[a0[..., 1]]
    fx, fy = np.clip(front[..., 0], 0, W - 1), np.clip(front[..., 1], 0, H - 1)
    tb = np.arange(T)[:, None, None], np.arange(B)[None, :, None]
    fcell = g0[tb[0], tb[1], fy, fx]                                               # [T,B,A,3] the cell in front, before the step
    ft, fs = fcell[..., 0], fcell[..., 2]
    live = a0[..., 4] == 0
    # other agents standing on the front cell before AND after the step (so the order of the moves does not matter)
    on_front = ((pos0[:, :, None, :, :] == front[:, :, :, None, :]).all(-1) &
                (a1[:, :, None, :, 2:4] == front[:, :, :, None, :]).all(-1))           # [T,B,A(i),A(j)]
    on_front &= ~np.eye(A, dtype=bool)
    term_on_front = (on_front & (a0[:, :, None, :, 4] != 0)).any(-1)
    overlappable = np.isin(ft, (1, 3, 8, 9)) | ((ft == 4) & (fs == 0))
    stayed = (a1[..., 2:4] == pos0).all(-1)
    fwd_blocked = (act == 2) & live & overlappable & on_front.any(-1) & stayed
    ev["forward_blocked_by_agent"] = int(fwd_blocked.sum()) if not spec.allow_agent_overlap else 0
    ev["forward_blocked_by_terminated_agent"] = int((fwd_blocked & term_on_front).sum()) if not spec.allow_agent_overlap else 0
    ev["drop_refused_agent_on_cell"] = int(((act == 4) & live & (a0[..., 5] != 1) & (ft == 1) & on_front.any(-1)
                                            & (a1[..., 5:8] == a0[..., 5:8]).all(-1)).sum())
    ev["terminated_action_ignored"] = int(((act == 0) | (act == 1)).__and__(~live).__and__(a1[..., 1] == a0[..., 1]).sum())
    ev["missing_action"] = int(((act < 0) & live).sum())
    ev["pickup"] = int(((a0[..., 5] == 1) & (a1[..., 5] != 1)).sum())
    door = (g0[..., 0] == 4) & (g1[..., 0] == 4)
    s0, s1 = g0[..., 2], g1[..., 2]
    ev["door_open_to_closed"] = int((door & (s0 == 0) & (s1 == 1)).sum())
    ev["door_closed_to_open"] = int((door & (s0 == 1) & (s1 == 0)).sum())
    ev["door_unlocked"] = int((door & (s0 == 2) & (s1 == 0)).sum())
    box_gone = (g0[..., 0] == 7) & (g1[..., 0] != 7)
    ev["filled_box_toggled"] = int((box_gone & (g1[..., 0] != 1)).sum())
    picked_boxes = ((a0[..., 5] == 1) & (a1[..., 5] == 7)).sum(-1)                # [T,B]
    ev["empty_box_toggled"] = int(((box_gone & (g1[..., 0] == 1)).sum((-1, -2)) > picked_boxes).sum())
    success = (rew > 0).any(-1)
    mode = spec.success_termination_mode
    ev[f"success_{mode}"] = int(success.sum())
    # lava: a live agent that stepped onto lava and ended the step terminated
    on_lava = g1[tb[0], tb[1], a1[..., 3], a1[..., 2]][..., 0] == 9
    lava = live & ~stayed & on_lava & (a1[..., 4] != 0)
    ev[f"lava_{spec.failure_termination_mode}"] = int(lava.sum())
    ev["truncated_with_success"] = int((trunc & success).sum())
    ev["joint_reward"] = int(((rew > 0).all(-1) & success).sum()) if spec.joint_reward and A > 1 else 0
    ev["agent_in_obs"] = int((z["obs"][..., 0] == 10).sum())
    ev["unseen_in_obs"] = int((z["obs"][..., 0] == 0).sum())
    return ev


def test_randstate_corpus_covers_the_dynamics():
    """The random-state corpus must hold every event below (in the reference's own recording) -- otherwise its pin is hollow."""
    from tests import util
    need = ["forward_blocked_by_agent", "forward_blocked_by_terminated_agent", "drop_refused_agent_on_cell",
            "terminated_action_ignored", "missing_action", "pickup", "door_open_to_closed", "door_closed_to_open", "door_unlocked",
            "filled_box_toggled", "empty_box_toggled", "success_any", "success_all", "lava_any", "lava_all",
            "truncated_with_success", "joint_reward", "agent_in_obs", "unseen_in_obs"]
    seen = dict.fromkeys(need, 0)
    for path in util.RANDSTATE_GOLDEN:
        z, d, spec = _randstate(path)
        for k, v in randstate_events(z, spec).items():
            seen[k] = seen.get(k, 0) + v
    missing = [k for k in need if seen[k] == 0]
    assert not missing, (missing, seen)
    print(seen)


def test_randstate_corpus_spans_the_shapes():
    from tests import util
    specs = [util.load_golden(p)[2] for p in util.RANDSTATE_GOLDEN]
    assert {1, 2, 3, 4, 5, 7, 16} <= {s.num_agents for s in specs}
    assert {3, 5, 7, 9, 11, 15} <= {s.view_size for s in specs}
    assert any(s.width != s.height for s in specs)
    for flag in ("see_through_walls", "allow_agent_overlap", "joint_reward"):
        assert {getattr(s, flag) for s in specs} == {False, True}, flag
    for mode in ("success_termination_mode", "failure_termination_mode"):
        assert {getattr(s, mode) for s in specs} == {"any", "all"}, mode
    assert (16, 16, 4, 7) in {(s.width, s.height, s.num_agents, s.view_size) for s in specs}
    assert (64, 64, 16, 9) in {(s.width, s.height, s.num_agents, s.view_size) for s in specs}
    assert any(s.env_kind == "blockedunlockpickup" for s in specs)
    assert sum(os.path.getsize(p) for p in util.RANDSTATE_GOLDEN) <= 1 << 20
