#!/usr/bin/env python3
"""Generate golden vectors by running the REAL reference (ini/multigrid) in the build container.

TEST INFRASTRUCTURE -- not product code.  Runs only where /root/reference exists (never on the GPU box):

    python oracle/gen_golden.py            # rewrites tests/golden/*.npz

The reference's four absent third-party packages are satisfied by `oracle/standins/` (this repo's own
stand-ins; see its README).  Every array written here is *data produced by the reference*: initial state
tensors, the post-reset bit-generator state, the action script, and per step the reference's outputs
(`MultiGridEnv.step`, multigrid/base.py:303-346) and post-step state.  No reference source is copied.

Array conventions in the .npz files (reference layouts, narrowed to the smallest lossless dtype):
    grid0        (W,H,3)   Grid.state after reset (+ scenario edits)       multigrid/core/grid.py:54
    agents0      (A,9)     AgentState rows after reset                     multigrid/core/agent.py:222-232
    rng0         (4,) u64  PCG64 [state_hi, state_lo, inc_hi, inc_lo] after reset returned (SURVEY A.6 trap)
    actions      (T,A) i8  -1 = agent key absent from the actions dict     multigrid/base.py:403-404
    order        (T,A)     handle_actions' random visiting order           multigrid/base.py:396-399
    obs0         (A,v,v,3) reset observation images                        multigrid/base.py:295
    obs          (T,A,v,v,3), direction (T,A), reward (T,A) f64, terminated (T,A), truncated (T,)
    grid         (T,W,H,3), agents (T,A,9)  post-step state
    rng_final    (4,) u64
    spec_json    JSON: constructor-level parameters needed to rebuild the EnvSpec
    resets_*.npz (record_resets: single resets from given generator states; product layout) hold other arrays:
                 lay_before / npr_before / lay_after / npr_after u64[N,5], grid0 u8[N,H,W,3], agents0 u8[N,A,8], obs0, target,
                 lay_halves / npr_halves, and the instrumentation tables calls / resamples / shuffles / key_draws / object_rooms
                 (see record_resets' docstring)
    conflict_*.npz (record_conflicts: constructed envs in which the visiting order decides the outcome) hold the arrays of
                 randstate_*.npz (record_random_states' docstring) and order / scenario / cluster_agents / cluster_block
    hook_order   (T,A) u8, only in the *_dictorder fixtures: the insertion order of the keys of the actions dict handed to
                 step() at step t (the RedBlueDoors / LockedHallway hooks iterate actions.items(), redbluedoors.py:176,
                 locked_hallway.py:210); every other fixture builds its dict in ascending agent order
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REFERENCE = os.environ.get("MGX_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.join(HERE, "standins"))

import numpy as np  # noqa: E402

import multigrid.envs as ref_envs  # noqa: E402
from multigrid.core.world_object import Ball, Box, Door, Floor, Key, Lava, Wall  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
_MAKE_COUNT = [0]
M64 = (1 << 64) - 1


def rng_words(gen) -> np.ndarray:
    st = gen.bit_generator.state["state"]
    s, inc = int(st["state"]), int(st["inc"])
    return np.array([s >> 64, s & M64, inc >> 64, inc & M64], dtype=np.uint64)


def clone_order(gen, n):
    """What handle_actions will draw next (base.py:396-399), without disturbing the env's generator."""
    if n == 1:
        return np.zeros(1, dtype=np.int64)
    bg = np.random.PCG64()
    bg.state = gen.bit_generator.state
    return np.random.Generator(bg).random(size=n).argsort()


def narrow(a):
    a = np.asarray(a)
    if a.dtype == np.bool_:
        return a.astype(np.uint8)
    if a.dtype.kind in "iu":
        lo, hi = (int(a.min()), int(a.max())) if a.size else (0, 0)
        if lo >= 0 and hi <= 255:
            return a.astype(np.uint8)
        if lo >= -128 and hi <= 127:
            return a.astype(np.int8)
        return a.astype(np.int32)
    return a


#: Box.contains (multigrid/core/world_object.py:574-605) is an attribute of the Python object: neither Grid.state nor the agent
#: rows show it.  The fixtures record it where the product's byte layouts carry it (include/mgx.h "BOX CONTENTS"): in the upper
#: bits of the box cell's STATE value, state | kind << 2 | colour << 5.  Every fixture without a filled box is unchanged by this.
_CONTENT_KIND = {"key": 1, "ball": 2, "goal": 3, "floor": 4, "lava": 5, "wall": 6, "door": 7}


def content_code(obj) -> int:
    inner = getattr(obj, "contains", None)
    if inner is None:
        return 0
    name = inner.type.value if hasattr(inner.type, "value") else str(inner.type)
    assert name in _CONTENT_KIND, f"box content {name!r} has no code"
    assert name != "door" or int(inner[2]) == 1, "a door in a box: closed and unlocked only"
    return _CONTENT_KIND[name] | (int(inner[1]) << 3)


def grid_with_contents(env) -> np.ndarray:
    """env.grid.state (W,H,3) + what the boxes lying on the grid hold."""
    st = env.grid.state.copy()
    for x, y in np.argwhere(st[..., 0] == 7):
        st[x, y, 2] |= content_code(env.grid.get(int(x), int(y))) << 2
    return st


def agents_with_contents(env) -> np.ndarray:
    """env.agent_states (A,9) + what the boxes being carried hold."""
    rows = np.asarray(env.agent_states).copy()
    for agent in env.agents:
        carried = agent.state.carrying
        if carried is not None and int(carried[0]) == 7:
            rows[agent.index, 8] |= content_code(carried) << 2
    return rows


def make_env(name, **kwargs):
    cls, cfg = ref_envs.CONFIGURATIONS[name]
    # pin the construction-time (layout) generator so regeneration is reproducible; see standins/gymnasium
    _MAKE_COUNT[0] += 1
    cls._default_seed = 0xC0FFEE + _MAKE_COUNT[0]
    return cls(**{**cfg, **kwargs})


def spec_of(env, kind, extra=None):
    d = dict(
        env_kind=kind,
        width=int(env.width), height=int(env.height), num_agents=int(env.num_agents),
        view_size=int(env.agents[0].view_size),
        see_through_walls=bool(env.agents[0].see_through_walls),
        allow_agent_overlap=bool(env.allow_agent_overlap),
        joint_reward=bool(env.joint_reward),
        success_termination_mode=str(env.success_termination_mode),
        failure_termination_mode=str(env.failure_termination_mode),
        max_steps=int(env.max_steps),
    )
    if kind == "blockedunlockpickup":
        d["target"] = [int(v) for v in np.asarray(env.obj)]
    if kind == "redbluedoors":
        d["blue_door"] = [int(v) for v in env.blue_door.cur_pos or door_pos(env, "blue")]
        d["red_door"] = [int(v) for v in env.red_door.cur_pos or door_pos(env, "red")]
    if kind == "lockedhallway":
        d["doors"] = sorted([int(x), int(y)] for x, y in np.argwhere(env.grid.state[..., 0] == 4))
        d["num_room_keys"] = len(env.rooms)          # rooms keyed by colour: what ends the episode (locked_hallway.py:222-225)
    d.update(extra or {})
    return d


def door_pos(env, color):
    ci = ["red", "green", "blue", "purple", "yellow", "grey"].index(color)
    st = env.grid.state
    (x, y), = np.argwhere((st[..., 0] == 4) & (st[..., 1] == ci))
    return int(x), int(y)


def record(fname, env, kind, seed, T, action_rng, p_missing=0.0, edit=None, script=None, note="", dict_orders=None):
    obs0, _ = env.reset(seed=seed)
    if edit is not None:
        edit(env)
        obs0 = env.gen_obs()
    A = env.num_agents
    rec = dict(
        grid0=narrow(grid_with_contents(env)),
        agents0=narrow(agents_with_contents(env)),
        rng0=rng_words(env.np_random),
        obs0=narrow(np.stack([obs0[i]["image"] for i in range(A)])),
        dir0=narrow(np.array([int(obs0[i]["direction"]) for i in range(A)])),
    )
    if script is not None:
        actions = np.asarray(script, dtype=np.int8)
        T = len(actions)
    else:
        actions = action_rng.integers(0, 7, size=(T, A)).astype(np.int8)
        if p_missing > 0:
            actions[action_rng.random((T, A)) < p_missing] = -1
    keys = ("order", "obs", "direction", "reward", "terminated", "truncated", "grid", "agents")
    log = {k: [] for k in keys}
    for t in range(T):
        log["order"].append(clone_order(env.np_random, A))
        key_order = range(A) if dict_orders is None else [int(i) for i in dict_orders[t]]
        act = {i: int(actions[t, i]) for i in key_order if actions[t, i] >= 0}
        obs, rew, term, trunc, _ = env.step(act)
        log["obs"].append(np.stack([obs[i]["image"] for i in range(A)]))
        log["direction"].append([int(obs[i]["direction"]) for i in range(A)])
        log["reward"].append([float(rew[i]) for i in range(A)])
        log["terminated"].append([bool(term[i]) for i in range(A)])
        log["truncated"].append(bool(trunc[0]))
        assert len(set(bool(trunc[i]) for i in range(A))) == 1
        log["grid"].append(grid_with_contents(env))
        log["agents"].append(agents_with_contents(env))
    rec["actions"] = actions
    if dict_orders is not None:
        rec["hook_order"] = np.asarray(dict_orders, dtype=np.uint8)[:T]
    for k in keys:
        arr = np.asarray(log[k])
        rec[k] = arr.astype(np.float64) if k == "reward" else narrow(arr)
    rec["rng_final"] = rng_words(env.np_random)
    rec["spec_json"] = np.array(json.dumps(spec_of(env, kind, dict(seed=seed, note=note))))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, fname + ".npz")
    np.savez_compressed(path, **rec)
    n_succ = int((rec["reward"] > 0).any(axis=1).sum())
    print(f"{fname:34s} T={T:4d} A={A:2d} grid={env.width}x{env.height} "
          f"success-steps={n_succ:3d} terminated-end={rec['terminated'][-1].tolist()} "
          f"{os.path.getsize(path) / 1024:.1f} KiB")


def sprinkle(density, seed, doors=True):
    """Scenario edit: scatter every object type over interior cells not under an agent (uses the
    reference's own WorldObj classes and Grid.set, multigrid/core/grid.py:78-100)."""
    colors = ["red", "green", "blue", "purple", "yellow", "grey"]

    def edit(env):
        r = np.random.default_rng(seed)
        agent_cells = {tuple(int(v) for v in a.state.pos) for a in env.agents}
        for x in range(1, env.width - 1):
            for y in range(1, env.height - 1):
                if (x, y) in agent_cells or env.grid.get(x, y) is not None:
                    continue
                if r.random() >= density:
                    continue
                c = colors[int(r.integers(6))]
                k = int(r.integers(9 if doors else 6))
                obj = [lambda: Lava(), lambda: Floor(c), lambda: Key(c), lambda: Ball(c), lambda: Box(c),
                       lambda: Wall(), lambda: Door(c), lambda: Door(c, is_locked=True),
                       lambda: Door(c, is_open=True)][k]()
                env.grid.set(x, y, obj)
    return edit


def main():
    # C1: the reference's own CPU-runnable case (BASELINE.json configs[0])
    record("empty8_a2_seed0", make_env("MultiGrid-Empty-8x8-v0", agents=2), "empty", 0, 256,
           np.random.default_rng(0), note="C1 plumbing case; actions default_rng(0).integers(0,7,(T,A))")
    # C2/C4 shape: Empty-16x16, 4 agents, view 7
    for seed in (1, 7):
        record(f"empty16_a4_seed{seed}", make_env("MultiGrid-Empty-16x16-v0", agents=4), "empty", seed, 300,
               np.random.default_rng(100 + seed), note="C2/C4 shape")
    # biased towards 'forward' so agents reach the goal: exercises on_success ('any') + reward value
    def fwd_script(T, A, seed):
        r = np.random.default_rng(seed)
        return r.choice([0, 1, 2, 2, 2, 2, 2, 5], size=(T, A)).astype(np.int8)
    record("empty6_a3_goal", make_env("MultiGrid-Empty-6x6-v0", agents=3), "empty", 3, None, None,
           script=fwd_script(120, 3, 5), note="goal reached under success 'any'; steps after termination")
    record("empty6_a3_goal_all_joint",
           make_env("MultiGrid-Empty-6x6-v0", agents=3, success_termination_mode="all", joint_reward=True),
           "empty", 4, None, None, script=fwd_script(200, 3, 6), note="success 'all' + joint reward")
    # every object type, doors in all 3 states, 5% missing actions
    record("empty16_a4_objects", make_env("MultiGrid-Empty-16x16-v0", agents=4), "empty", 11, 400,
           np.random.default_rng(211), p_missing=0.05, edit=sprinkle(0.30, 5), note="all object types")
    record("empty8_a3_dense", make_env("MultiGrid-Empty-8x8-v0", agents=3), "empty", 12, 400,
           np.random.default_rng(212), p_missing=0.05, edit=sprinkle(0.45, 6), note="dense pickup/drop/toggle")
    # lava with failure 'any' and 'all'
    record("empty8_a3_lava_any",
           make_env("MultiGrid-Empty-8x8-v0", agents=3, failure_termination_mode="any"), "empty", 13, None, None,
           edit=sprinkle(0.25, 7, doors=False), script=fwd_script(150, 3, 8), note="lava, failure 'any'")
    record("empty8_a3_lava_all", make_env("MultiGrid-Empty-8x8-v0", agents=3), "empty", 14, None, None,
           edit=sprinkle(0.25, 9, doors=False), script=fwd_script(150, 3, 10), note="lava, failure 'all'")
    # no agent overlap, view 5, random starts
    record("emptyrand6_a3_nooverlap_v5",
           make_env("MultiGrid-Empty-Random-6x6-v0", agents=3, allow_agent_overlap=False, agent_view_size=5),
           "empty", 21, 300, np.random.default_rng(221), p_missing=0.05, note="allow_agent_overlap=False, v=5")
    # single agent (no RNG draw, no overlay), see_through_walls
    record("empty8_a1_seethrough", make_env("MultiGrid-Empty-8x8-v0", agents=1, see_through_walls=True),
           "empty", 22, 200, np.random.default_rng(222), edit=sprinkle(0.3, 11), note="A=1, see_through_walls")
    record("empty8_a1_walls", make_env("MultiGrid-Empty-8x8-v0", agents=1),
           "empty", 23, 200, np.random.default_rng(223), edit=sprinkle(0.3, 12), note="A=1, occlusion")
    # 5 agents, v=9, success all / failure any / joint reward / random starts
    record("empty16_a5_v9_modes",
           make_env("MultiGrid-Empty-16x16-v0", agents=5, agent_view_size=9, agent_start_pos=None,
                    success_termination_mode="all", failure_termination_mode="any", joint_reward=True),
           "empty", 31, 300, np.random.default_rng(231), p_missing=0.05, edit=sprinkle(0.15, 13),
           note="v=9, modes")
    # tiny view / large view
    record("empty8_a2_v3", make_env("MultiGrid-Empty-8x8-v0", agents=2, agent_view_size=3), "empty", 32, 150,
           np.random.default_rng(232), edit=sprinkle(0.3, 14), note="v=3")
    record("empty16_a2_v11", make_env("MultiGrid-Empty-16x16-v0", agents=2, agent_view_size=11,
                                      agent_start_pos=None), "empty", 33, 150,
           np.random.default_rng(233), edit=sprinkle(0.25, 15), note="v=11")
    # max_steps truncation boundary
    record("empty5_a2_trunc", make_env("MultiGrid-Empty-5x5-v0", agents=2, max_steps=20), "empty", 34, 40,
           np.random.default_rng(234), note="truncation at step 20, stepping beyond")
    # C5 shape: 64x64, 16 agents, view 9
    record("empty64_a16_v9", make_env("MultiGrid-Empty-8x8-v0", size=64, agents=16, agent_view_size=9,
                                      agent_start_pos=None), "empty", 41, 60,
           np.random.default_rng(241), edit=sprinkle(0.08, 16), note="C5 shape")
    # C3: BlockedUnlockPickup (RoomGrid draws from the seeded stream inside reset -> rng0 snapshot matters)
    for A, seed in ((2, 51), (3, 52)):
        record(f"bup_a{A}_seed{seed}", make_env("MultiGrid-BlockedUnlockPickup-v0", agents=A),
               "blockedunlockpickup", seed, 300, np.random.default_rng(250 + A), p_missing=0.03, note="C3")

    # C3 with the post-step success hook firing: teleport agent 0 next to the target box, facing it
    def next_to_box(env):
        bx, by = env.obj.cur_pos
        for d, (dx, dy) in enumerate([(1, 0), (0, 1), (-1, 0), (0, -1)]):
            x, y = bx - dx, by - dy
            if env.grid.get(x, y) is None:
                env.agents[0].state.pos = (x, y)
                env.agents[0].state.dir = d
                return
        raise RuntimeError("box is boxed in")
    hook = np.array([[6, 2]] * 3 + [[3, 0]] + [[2, 1], [4, 2], [3, 5], [5, 3], [0, 4]] * 4, dtype=np.int8)
    record("bup_a2_hook", make_env("MultiGrid-BlockedUnlockPickup-v0", agents=2), "blockedunlockpickup",
           53, None, None, edit=next_to_box, script=hook, note="post-step hook: carrying target box -> success")

    # scripted key / locked-door protocol (world_object.py:458-474): wrong key, no key, unlock, close, reopen
    def key_and_doors(env):
        env.grid.set(2, 1, Key("blue"))
        env.grid.set(3, 1, Door("blue", is_locked=True))
        env.grid.set(2, 2, Door("red", is_locked=True))
        for y in range(2, 7):
            env.grid.set(3, y, Wall())
    script = [[3, 6], [2, 2], [6, 5], [1, 6], [5, 6], [0, 6], [5, 6], [6, 5], [6, 5], [2, 2], [2, 6], [4, 6],
              [6, 5]]
    script += np.random.default_rng(77).integers(0, 7, size=(80, 2)).tolist()
    record("empty8_a2_unlock", make_env("MultiGrid-Empty-8x8-v0", agents=2), "empty", 61, None, None,
           edit=key_and_doors, script=script, note="scripted unlock / wrong key / close / reopen")

    record_layouts()
    record_wrappers()
    record_hook_envs()
    record_dict_order()
    record_custom()          # (last: every make_env() before it keeps the construction seed it always had)
    record_custom_steps()    # (round 5, behind everything older for the same reason)
    record_box_rollout()
    import custom_envs       # (round 6, likewise: the RoomGrid subclass of tests/custom_envs.py)
    record_custom(custom_envs.CASES_R6)
    record_custom_steps(custom_envs.STEP_CASES_R6)
    record_edge()            # (behind everything older for the same reason)
    record_random_states()   # (constructs no registered env: every make_env() above keeps its construction seed)
    record_resets()          # (likewise; both generators' states are set before every recorded reset)
    record_reset_chains()
    record_lh_12rooms()      # (a construction seed of its own: nothing above moves)
    record_conflicts()       # (constructs no registered env either)


def face(env, i, target_xy, carrying=None):
    """Teleport agent i next to `target_xy`, facing it (first free side)."""
    tx, ty = target_xy
    for d, (dx, dy) in enumerate([(1, 0), (0, 1), (-1, 0), (0, -1)]):
        x, y = tx - dx, ty - dy
        if 0 < x < env.width - 1 and 0 < y < env.height - 1 and env.grid.get(x, y) is None:
            env.agents[i].state.pos = (x, y)
            env.agents[i].state.dir = d
            if carrying is not None:
                env.agents[i].state.carrying = carrying
            return
    raise RuntimeError("no free side")


def record_edge():
    """The largest grid the product accepts (sides <= 255) with the largest view: three agents on the far
    edges -- the last interior column, the last interior row and the far corner (the goal taken off it) -- turned to face the
    outer wall, objects of every kind in a band along those edges, random actions.  Pins the oracle itself where the views hang
    over the far walls, at coordinates beyond 128."""
    colors = ["red", "green", "blue", "purple", "yellow", "grey"]

    def edges(env):
        W, H = env.width, env.height
        env.grid.set(W - 2, H - 2, None)
        face(env, 0, (W - 1, H // 2))
        face(env, 1, (W // 2, H - 1))
        env.agents[2].state.pos = (W - 2, H - 2)
        env.agents[2].state.dir = 0
        r = np.random.default_rng(17)
        agent_cells = {tuple(int(v) for v in a.state.pos) for a in env.agents}
        for x in range(1, W - 1):
            for y in range(1, H - 1):
                if min(W - 2 - x, H - 2 - y) >= 9 or (x, y) in agent_cells or r.random() >= 0.2:
                    continue
                c = colors[int(r.integers(6))]
                env.grid.set(x, y, [Lava, lambda: Floor(c), lambda: Key(c), lambda: Ball(c), lambda: Box(c), Wall,
                                    lambda: Door(c), lambda: Door(c, is_open=True)][int(r.integers(8))]())
    record("empty255_a3_v15_edges", make_env("MultiGrid-Empty-8x8-v0", size=255, agents=3, agent_view_size=15), "empty", 91,
           12, np.random.default_rng(291), edit=edges, note="largest grid and view; agents on the far edges, facing out")


def record_hook_envs():
    """Section 8f-4: RedBlueDoors (envs/redbluedoors.py:170-187, incl. the stale-grid quirk Q9), LockedHallway
    (envs/locked_hallway.py:203-227) and Playground (no hook; RoomGrid layout) -- rollouts of the real reference."""
    from multigrid.core.world_object import Key
    T, L, R, F, P, D, G, N = 5, 0, 1, 2, 3, 4, 5, 6   # toggle, left, right, forward, pickup, drop, toggle(again), done

    def rbd_success(env):
        face(env, 0, door_pos(env, "red")); face(env, 1, door_pos(env, "blue"))
    record("rbd_a2_success", make_env("MultiGrid-RedBlueDoors-8x8-v0", agents=2), "redbluedoors", 71, None, None,
           edit=rbd_success, script=[[T, N], [N, T], [N, T], [T, T], [F, F], [N, T]],
           note="red then blue: success; hook keeps firing for terminated agents")

    def rbd_failure(env):
        face(env, 1, door_pos(env, "blue"))
        bx, by = door_pos(env, "blue")
        env.agents[0].state.pos = (bx - 1, by); env.agents[0].state.dir = 0
    for mode in ("any", "all"):
        record(f"rbd_a2_failure_{mode}",
               make_env("MultiGrid-RedBlueDoors-8x8-v0", agents=2, failure_termination_mode=mode), "redbluedoors", 72,
               None, None, edit=rbd_failure,
               script=[[N, T], [F, N], [T, N], [F, T], [T, N], [F, F], [T, T], [F, F], [L, T], [T, N]],
               note="blue first: failure; the blue door object closes while grid.state keeps saying open (Q9)")
    record("rbd_a3_random", make_env("MultiGrid-RedBlueDoors-6x6-v0", agents=3, failure_termination_mode="all"),
           "redbluedoors", 73, 400, np.random.default_rng(373), p_missing=0.05, note="random rollout")

    def lh_unlock(env):
        doors = sorted((int(x), int(y)) for x, y in np.argwhere(env.grid.state[..., 0] == 4))
        colors = ["red", "green", "blue", "purple", "yellow", "grey"]
        for i, (x, y) in enumerate(doors[:env.num_agents]):
            face(env, i, (x, y), carrying=Key(colors[int(env.grid.state[x, y, 1])]))
    for name, A, jr in (("MultiGrid-LockedHallway-2Rooms-v0", 2, True), ("MultiGrid-LockedHallway-2Rooms-v0", 2, False),
                        ("MultiGrid-LockedHallway-6Rooms-v0", 3, True)):
        rooms = name.split("-")[2]
        record(f"lh_{rooms.lower()}_a{A}_{'joint' if jr else 'own'}", make_env(name, agents=A, joint_reward=jr),
               "lockedhallway", 74 + A, None, None, edit=lh_unlock,
               script=[[N] * A, [T] + [N] * (A - 1), [T] * A, [T] * A, [F] * A, [T] * A, [L] * A, [T] * A] +
                      np.random.default_rng(5).integers(0, 7, size=(30, A)).tolist(),
               note="unlock with key: reward accumulates; all doors unlocked -> returned terminations only")
    record("lh_4rooms_a2_random", make_env("MultiGrid-LockedHallway-4Rooms-v0", agents=2), "lockedhallway", 77, 300,
           np.random.default_rng(377), p_missing=0.05, note="random rollout")
    record("playground_a3", make_env("MultiGrid-Playground-v0", agents=3), "empty", 78, 100,
           np.random.default_rng(378), p_missing=0.05, note="Playground: no hook, 19x19 RoomGrid layout, max_steps 100")
    # more rooms than colours (not a registered id: the class called directly): doors repeat colours, len(self.rooms) < doors
    _MAKE_COUNT[0] += 1
    ref_envs.LockedHallwayEnv._default_seed = 0xC0FFEE + _MAKE_COUNT[0]
    record("lh_8rooms_a8_joint", ref_envs.LockedHallwayEnv(num_rooms=8, agents=8, joint_reward=True), "lockedhallway", 81,
           None, None, edit=lh_unlock,
           script=[[N] * 8, [T] + [N] * 7, [T] * 8, [T] * 8, [F] * 8, [T] * 8, [L] * 8, [T] * 8] +
                  np.random.default_rng(6).integers(0, 7, size=(30, 8)).tolist(),
           note="8 rooms, 6 colours: rooms dict keyed by colour; every agent unlocks a door")


def record_dict_order():
    """The env hooks visit the agents in the insertion order of the caller's dict (redbluedoors.py:176, locked_hallway.py:210).
    Cases where that order decides the result, plus random rollouts with a random key order every step."""
    from multigrid.core.world_object import Key
    T, L, R, F, P, D, N = 5, 0, 1, 2, 3, 4, 6

    # RedBlueDoors, failure 'all', three agents stacked in front of the CLOSED blue door, all toggle in one step: the door
    # goes closed -> open -> closed -> open in handle_actions, then the hook fails the FIRST toggler in dict order only (it
    # closes the blue door object, so the next ones find it closed)
    def rbd_three(env):
        face(env, 0, door_pos(env, "blue"))
        for i in (1, 2):
            env.agents[i].state.pos = env.agents[0].state.pos
            env.agents[i].state.dir = env.agents[0].state.dir
    for tag, orders in (("rev", [[2, 1, 0]] * 6), ("mid", [[1, 2, 0], [1, 0, 2], [2, 0, 1], [0, 2, 1], [1, 2, 0], [2, 1, 0]])):
        record(f"rbd_a3_dictorder_{tag}",
               make_env("MultiGrid-RedBlueDoors-8x8-v0", agents=3, failure_termination_mode="all"), "redbluedoors", 91, None, None,
               edit=rbd_three, script=[[T, T, T], [N, N, N], [T, T, T], [T, N, T], [T, T, N], [T, T, T]], dict_orders=orders,
               note="three togglers of the blue door in one step: the first in DICT order fails (failure 'all')")

    # LockedHallway, own rewards: agent 0 (with the key) and agent 1 face the same locked door from the hallway and both toggle:
    # whoever comes first in dict order is paid for the unlock
    def lh_two(env):
        doors = sorted((int(x), int(y)) for x, y in np.argwhere(env.grid.state[..., 0] == 4))
        colors = ["red", "green", "blue", "purple", "yellow", "grey"]
        x, y = doors[0]
        face(env, 0, (x, y), carrying=Key(colors[int(env.grid.state[x, y, 1])]))
        env.agents[1].state.pos = env.agents[0].state.pos
        env.agents[1].state.dir = env.agents[0].state.dir
    for tag, orders in (("rev", [[1, 0]] * 8), ("fwd", [[0, 1]] * 8)):
        record(f"lh_2rooms_a2_dictorder_{tag}", make_env("MultiGrid-LockedHallway-2Rooms-v0", agents=2, joint_reward=False),
               "lockedhallway", 92, None, None, edit=lh_two,
               script=[[N, N], [T, T], [T, T], [T, N], [N, T], [T, T], [F, F], [T, T]], dict_orders=orders,
               note="two togglers of one door in one step: the first in DICT order is paid (joint_reward=False)")

    # random rollouts, a random permutation of the keys every step, agents kept near the doors by a biased action mix
    def perm_orders(T_, A, seed):
        r = np.random.default_rng(seed)
        return np.stack([r.permutation(A) for _ in range(T_)]).astype(np.uint8)

    def rbd_near(env):
        face(env, 0, door_pos(env, "blue")); face(env, 1, door_pos(env, "red"))
        env.agents[2].state.pos = env.agents[0].state.pos; env.agents[2].state.dir = env.agents[0].state.dir
    tog = np.random.default_rng(94).choice([T, T, T, L, R, F, N], size=(200, 3)).astype(np.int8)
    record("rbd_a3_random_dictorder",
           make_env("MultiGrid-RedBlueDoors-6x6-v0", agents=3, failure_termination_mode="all", success_termination_mode="all"),
           "redbluedoors", 93, None, None, edit=rbd_near, script=tog, dict_orders=perm_orders(200, 3, 95),
           note="toggle-heavy random rollout, random dict order every step")
    record("lh_4rooms_a3_random_dictorder", make_env("MultiGrid-LockedHallway-4Rooms-v0", agents=3, joint_reward=False),
           "lockedhallway", 96, 300, np.random.default_rng(397), p_missing=0.05, dict_orders=perm_orders(300, 3, 98),
           note="random rollout, random dict order every step")

    # more than 6 rooms with an EVEN room size -- the doors sit at (top + bottom) // 2 = row (rs-1) + (rs-1)//2
    def lh_unlock(env):
        doors = sorted((int(x), int(y)) for x, y in np.argwhere(env.grid.state[..., 0] == 4))
        colors = ["red", "green", "blue", "purple", "yellow", "grey"]
        for i, (x, y) in enumerate(doors[:env.num_agents]):
            face(env, i, (x, y), carrying=Key(colors[int(env.grid.state[x, y, 1])]))
    for rs in (4, 6):
        _MAKE_COUNT[0] += 1
        ref_envs.LockedHallwayEnv._default_seed = 0xC0FFEE + _MAKE_COUNT[0]
        record(f"lh_8rooms_rs{rs}_a4", ref_envs.LockedHallwayEnv(num_rooms=8, room_size=rs, agents=4, joint_reward=True),
               "lockedhallway", 99, None, None, edit=lh_unlock,
               script=[[N] * 4, [T] + [N] * 3, [T] * 4, [T] * 4, [F] * 4, [T] * 4, [L] * 4, [T] * 4] +
                      np.random.default_rng(7).integers(0, 7, size=(30, 4)).tolist(),
               note=f"8 rooms of even size {rs}: mid-wall doors at (top + bottom) // 2")


def record_lh_12rooms():
    """LockedHallway with 12 rooms of size 4: the geometric door format with doors 8-11, whose unlock bits are the second byte
    of the mask (include/mgx.h: aux[2]).  Agent 0 stands at door 0 (row 0, left), agents 1 and 2 together at door 9 (row 4, right),
    each with the door's key; after the scripted unlocks agent 0 is in reach of more doors by the random tail.  A random permutation
    of the dict's keys every step.  The construction seed is a constant of its own, so the function can run alone
    (`python oracle/gen_golden.py lh_12rooms`) and no other fixture's seed moves."""
    from multigrid.core.world_object import Key
    T, L, F, N = 5, 0, 2, 6
    colors = ["red", "green", "blue", "purple", "yellow", "grey"]
    rs = 4

    def door_xy(k):
        return ((rs - 1) * (1 + k % 2), (k // 2) * (rs - 1) + (rs - 1) // 2)

    def edit(env):
        for i, k in ((0, 0), (1, 9)):
            x, y = door_xy(k)
            assert env.grid.state[x, y, 0] == 4
            face(env, i, (x, y), carrying=Key(colors[int(env.grid.state[x, y, 1])]))
        x, y = door_xy(9)
        env.agents[2].state.pos = env.agents[1].state.pos
        env.agents[2].state.dir = env.agents[1].state.dir
        env.agents[2].state.carrying = Key(colors[int(env.grid.state[x, y, 1])])
    ref_envs.LockedHallwayEnv._default_seed = 0xC0FFEE + 0x1200
    r = np.random.default_rng(12)
    orders = np.stack([r.permutation(3) for _ in range(40)]).astype(np.uint8)
    record("lh_12rooms_rs4_a3_joint", ref_envs.LockedHallwayEnv(num_rooms=12, room_size=rs, agents=3, joint_reward=True),
           "lockedhallway", 112, None, None, edit=edit,
           script=[[N] * 3, [T, N, N], [N, T, T], [T] * 3, [F] * 3, [T] * 3, [L] * 3, [T] * 3] +
                  np.random.default_rng(8).choice([T, T, F, L, 1, N], size=(32, 3)).tolist(),
           dict_orders=orders, note="12 rooms of size 4: doors 0 and 9 unlocked, the mask crosses its first byte")


def record_wrappers():
    """OneHotObsWrapper / FullyObsWrapper outputs of the real reference (multigrid/wrappers.py:17-190) along a short
    rollout with every object type present."""
    from multigrid.wrappers import FullyObsWrapper, OneHotObsWrapper
    for fname, kw in (("wrappers_empty8_a3", dict(agents=3)), ("wrappers_empty16_a4_v5", dict(size=16, agents=4, agent_view_size=5))):
        base = make_env("MultiGrid-Empty-8x8-v0", **kw)
        base.reset(seed=9)
        sprinkle(0.3, 21)(base)
        A = base.num_agents
        oh, fo = OneHotObsWrapper(base), FullyObsWrapper(base)
        ar = np.random.default_rng(4)
        rec = dict(obs=[], one_hot=[], full=[], grid=[], agents=[])
        for t in range(40):
            act = {i: int(a) for i, a in enumerate(ar.integers(0, 7, size=A))}
            base.step(act)
            raw = base.gen_obs()
            rec["obs"].append(np.stack([raw[i]["image"] for i in range(A)]))
            o1 = oh.observation(base.gen_obs())
            rec["one_hot"].append(np.stack([o1[i]["image"] for i in range(A)]))
            o2 = fo.observation(base.gen_obs())
            assert all(o2[i]["image"] is o2[0]["image"] for i in range(A))
            rec["full"].append(np.array(o2[0]["image"]))
            rec["grid"].append(base.grid.state.copy()); rec["agents"].append(np.asarray(base.agent_states).copy())
        out = {k: narrow(np.asarray(v)) for k, v in rec.items()}
        out["spec_json"] = np.array(json.dumps(spec_of_noreset(base, "empty")))
        path = os.path.join(OUT, fname + ".npz")
        np.savez_compressed(path, **out)
        print(f"{fname:34s} one_hot{out['one_hot'].shape} full{out['full'].shape} {os.path.getsize(path) / 1024:.1f} KiB")


def record_layouts():
    """Layout / reset parity fixtures: a sequence of resets (seeded and unseeded, with steps in between) of one
    env object whose construction-time generator is known.  Pins multigrid_amd/layouts.py + MultiGridEnv.reset
    against multigrid/base.py:250-301, envs/empty.py:151-170, envs/blockedunlockpickup.py:142-164."""
    cases = [
        ("layout_bup_a2", "MultiGrid-BlockedUnlockPickup-v0", dict(agents=2), "blockedunlockpickup"),
        ("layout_bup_a3", "MultiGrid-BlockedUnlockPickup-v0", dict(agents=3), "blockedunlockpickup"),
        ("layout_emptyrandom6_a3", "MultiGrid-Empty-Random-6x6-v0", dict(agents=3), "empty"),
        ("layout_empty8_a2", "MultiGrid-Empty-8x8-v0", dict(agents=2), "empty"),
        ("layout_rbd8_a2", "MultiGrid-RedBlueDoors-8x8-v0", dict(agents=2), "redbluedoors"),
        ("layout_lh4_a2", "MultiGrid-LockedHallway-4Rooms-v0", dict(agents=2), "lockedhallway"),
        ("layout_playground_a2", "MultiGrid-Playground-v0", dict(agents=2), "empty"),
    ]
    for fname, name, kw, kind in cases:
        env = make_env(name, **kw)
        construct_seed = type(env)._default_seed
        A = env.num_agents
        reset_seeds = [5, -1, -1, 17, -1, 123456789, -1, -1]
        ar = np.random.default_rng(99)
        rec = dict(construct_seed=np.array(construct_seed), reset_seeds=np.array(reset_seeds),
                   spec_json=np.array(json.dumps(spec_of_noreset(env, kind))))
        grids, agents, rngs, obs0s, missions, acts_all, targets = [], [], [], [], [], [], []
        for k, sd in enumerate(reset_seeds):
            obs, _ = env.reset(seed=None if sd < 0 else sd)
            grids.append(env.grid.state.copy()); agents.append(np.asarray(env.agent_states).copy())
            rngs.append(rng_words(env.np_random))
            obs0s.append(np.stack([obs[i]["image"] for i in range(A)]))
            # mission_space.seed(None) draws OS entropy (base.py:272): only seeded resets have a reproducible mission
            missions.append(str(obs[0]["mission"]) if sd >= 0 else "<unseeded>")
            targets.append([int(v) for v in np.asarray(env.obj)] if kind == "blockedunlockpickup" else [0, 0, 0])
            acts = ar.integers(0, 7, size=(5, A)).astype(np.int8)
            acts_all.append(acts)
            for t in range(5):
                env.step({i: int(acts[t, i]) for i in range(A)})
        rec.update(grid0=narrow(np.asarray(grids)), agents0=narrow(np.asarray(agents)), rng0=np.asarray(rngs),
                   obs0=narrow(np.asarray(obs0s)), missions=np.array(missions), actions=np.asarray(acts_all),
                   targets=narrow(np.asarray(targets)))
        path = os.path.join(OUT, fname + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{fname:34s} resets={len(reset_seeds)} missions={sorted(set(missions))[:2]} "
              f"{os.path.getsize(path) / 1024:.1f} KiB")


def record_custom(cases=None):
    """User-defined envs written against the reference's extension point, `_gen_grid` + `put_obj` / `place_obj` / `place_agent` /
    `Grid.wall_rect / horz_wall / vert_wall` / the WorldObj classes (multigrid/base.py:229-247, 604-697; core/grid.py:78-195;
    core/world_object.py:279-616).  The class bodies are this repo's own (tests/custom_envs.py) and run here over the REAL
    reference; the same bodies run over multigrid_amd in tests/test_custom_envs.py.  Same layout as the reset fixtures above,
    plus the five steps after every reset with their outputs."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import custom_envs
    classes = custom_envs.define(custom_envs.multigrid_namespace())
    for fname, (cname, kw) in (custom_envs.CASES if cases is None else cases).items():
        cls = classes[cname]
        _MAKE_COUNT[0] += 1
        cls._default_seed = 0xC0FFEE + _MAKE_COUNT[0]
        env = cls(**kw)
        construct_seed = cls._default_seed
        A = env.num_agents
        reset_seeds = [3, -1, 44, -1, -1, 2024]
        ar = np.random.default_rng(7)
        rec = dict(construct_seed=np.array(construct_seed), reset_seeds=np.array(reset_seeds),
                   spec_json=np.array(json.dumps(spec_of_noreset(env, "empty"))))
        grids, agents, rngs, obs0s, acts_all, obs_s, rew_s, term_s = [], [], [], [], [], [], [], []
        for k, sd in enumerate(reset_seeds):
            obs, _ = env.reset(seed=None if sd < 0 else sd)
            grids.append(env.grid.state.copy()); agents.append(np.asarray(env.agent_states).copy())
            rngs.append(rng_words(env.np_random))
            obs0s.append(np.stack([obs[i]["image"] for i in range(A)]))
            acts = ar.choice([0, 1, 2, 2, 2, 3, 4, 5, 6], size=(5, A)).astype(np.int8)
            acts_all.append(acts)
            o_k, r_k, t_k = [], [], []
            for t in range(5):
                o, r, tm, tr, _ = env.step({i: int(acts[t, i]) for i in range(A)})
                o_k.append(np.stack([o[i]["image"] for i in range(A)]))
                r_k.append([float(r[i]) for i in range(A)]); t_k.append([bool(tm[i]) for i in range(A)])
            obs_s.append(o_k); rew_s.append(r_k); term_s.append(t_k)
        rec.update(grid0=narrow(np.asarray(grids)), agents0=narrow(np.asarray(agents)), rng0=np.asarray(rngs),
                   obs0=narrow(np.asarray(obs0s)), actions=np.asarray(acts_all), obs_steps=narrow(np.asarray(obs_s)),
                   reward_steps=np.asarray(rew_s, dtype=np.float64), terminated_steps=narrow(np.asarray(term_s)))
        path = os.path.join(OUT, fname + ".npz")
        np.savez_compressed(path, **rec)
        ntypes = sorted(set(int(v) for v in np.asarray(grids)[..., 0].ravel()))
        print(f"{fname:34s} resets={len(reset_seeds)} cell types seen={ntypes} {os.path.getsize(path) / 1024:.1f} KiB")


def record_custom_steps(cases=None):
    """User-defined envs stepped for whole episodes over the REAL reference (tests/custom_envs.py: STEP_CASES): boxes that hold
    things (Box.contains, world_object.py:574-605) and a `step` override that ends episodes through `on_success` / `on_failure`
    (base.py:478-532) the way the reference's own envs do.  Per reset: the initial state, then every step's actions, outputs and
    post-step state (box contents folded into the state values, see grid_with_contents)."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import custom_envs
    classes = custom_envs.define(custom_envs.multigrid_namespace())
    for fname, (cname, kw, T) in (custom_envs.STEP_CASES if cases is None else cases).items():
        cls = classes[cname]
        _MAKE_COUNT[0] += 1
        cls._default_seed = 0xC0FFEE + _MAKE_COUNT[0]
        env = cls(**kw)
        A = env.num_agents
        reset_seeds = [11, -1, 5, 77]
        ar = np.random.default_rng(13)
        rec = dict(construct_seed=np.array(cls._default_seed), reset_seeds=np.array(reset_seeds),
                   spec_json=np.array(json.dumps(spec_of_noreset(env, "empty"))))
        keys = ("grid0", "agents0", "rng0", "obs0", "actions", "obs", "reward", "terminated", "truncated", "grid", "agents")
        log = {k: [] for k in keys}
        events = dict(success=0, failure=0, opened=0)
        for sd in reset_seeds:
            obs, _ = env.reset(seed=None if sd < 0 else sd)
            log["grid0"].append(grid_with_contents(env)); log["agents0"].append(agents_with_contents(env))
            log["rng0"].append(rng_words(env.np_random))
            log["obs0"].append(np.stack([obs[i]["image"] for i in range(A)]))
            # walk, pick up, drop and toggle a lot: boxes get opened and carried, balls fetched, the trap door opened
            acts = ar.choice(7, size=(T, A), p=[0.12, 0.12, 0.36, 0.12, 0.08, 0.17, 0.03]).astype(np.int8)
            acts[ar.random((T, A)) < 0.04] = -1
            if cname == "BoxTreasureEnv":
                acts[0, 0] = 5                                   # agent 0 starts facing the key box: open it, take the key
                acts[1, 0] = 3
            ep = {k: [] for k in ("obs", "reward", "terminated", "truncated", "grid", "agents")}
            for t in range(T):
                forced = custom_envs.intervene(cname, env, t)          # (tests/custom_envs.py: the replaying tests make the same call)
                for i, a_i in (forced or {}).items():
                    acts[t, i] = a_i
                nbox = int((env.grid.state[..., 0] == 7).sum())
                o, r, tm, tr, _ = env.step({i: int(acts[t, i]) for i in range(A) if acts[t, i] >= 0})
                ep["obs"].append(np.stack([o[i]["image"] for i in range(A)]))
                ep["reward"].append([float(r[i]) for i in range(A)]); ep["terminated"].append([bool(tm[i]) for i in range(A)])
                ep["truncated"].append(bool(tr[0]))
                ep["grid"].append(grid_with_contents(env)); ep["agents"].append(agents_with_contents(env))
                events["success"] += any(float(r[i]) > 0 for i in range(A))
                events["failure"] += any(bool(tm[i]) and float(r[i]) == 0 for i in range(A)) and not any(float(r[i]) > 0 for i in range(A))
                carried = sum(a.state.carrying is not None and int(a.state.carrying[0]) == 7 for a in env.agents)
                events["opened"] += int(nbox > int((env.grid.state[..., 0] == 7).sum()) + carried)
            log["actions"].append(acts)
            for k, v in ep.items():
                log[k].append(v)
        for k in keys:
            arr = np.asarray(log[k])
            rec[k] = arr.astype(np.float64) if k == "reward" else (arr if k in ("rng0", "actions") else narrow(arr))
        path = os.path.join(OUT, fname + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{fname:34s} episodes={len(reset_seeds)} x {T} steps events={events} {os.path.getsize(path) / 1024:.1f} KiB")


def record_box_rollout():
    """A rollout fixture in the format of `record` from the BoxTreasureEnv of tests/custom_envs.py: replayed by every golden test
    (oracle, host rules, the HIP kernels through the C ABI) like the fixtures of the reference's own envs.  Agent 0 opens the box
    that holds the purple key, takes the key, walks to the locked purple door and unlocks it (scripted); the others act at random
    (toggle / pickup / drop heavy), so boxes are opened, carried and opened elsewhere."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import custom_envs
    cls = custom_envs.define(custom_envs.multigrid_namespace())["BoxTreasureEnv"]
    _MAKE_COUNT[0] += 1
    cls._default_seed = 0xC0FFEE + _MAKE_COUNT[0]
    env = cls(size=9, agents=3)
    T = 160
    ar = np.random.default_rng(31)
    script = ar.choice(7, size=(T, 3), p=[0.12, 0.12, 0.36, 0.12, 0.08, 0.17, 0.03]).astype(np.int8)
    # agent 0: (1, 6) facing down at the key box (1, 7): toggle (box -> key), pickup, turn left (-> facing right/east), forward x3 to
    # (4 - 1, 6)... the door sits at (4, 4): up two cells first
    env.reset(seed=9)
    assert tuple(int(v) for v in env.agents[0].state.pos) == (1, 6) and int(env.agents[0].state.dir) == 1
    plan = [5, 3, 0, 0, 2, 2, 1, 2, 2, 5, 2, 2]      # toggle, pickup, left, left (facing up), fwd, fwd (1,4), right (facing east), fwd, fwd (3,4), toggle door, fwd, fwd
    script[:len(plan), 0] = plan
    record("boxkey_a3", env, "empty", 9, T, None, script=script,
           note="BoxTreasureEnv (tests/custom_envs.py): boxes that hold a key / ball / goal / door / lava; agent 0 opens the key box, "
                "takes the key and unlocks the purple door")


#: product box-content kind (include/mgx.h "BOX CONTENTS") -> (Type index, state) of the object the box holds; the inverse of
#: content_code (a door comes out of a box closed and unlocked)
_CONTENT_CELL = {1: (5, 0), 2: (6, 0), 3: (8, 0), 4: (3, 0), 5: (9, 0), 6: (2, 0), 7: (4, 1)}

#: The random-state corpus (tests/golden/randstate_*.npz): batches of tests.util.random_state -- stacked agents, terminated agents
#: in the middle of the grid, agents on goals / lava, objects carried from the start, doors in every state, arbitrary PCG64 states
#: and step counts up to max_steps - 1 -- each loaded into the REAL reference and stepped there.
#: (name, EnvSpec keywords, batch, steps, random_state keywords)
RANDSTATE_SPECS = [
    ("randstate_7x5_a1_v3_see", dict(width=7, height=5, num_agents=1, view_size=3, max_steps=10, see_through_walls=True),
     32, 16, dict(density=0.35, carry_p=0.5)),
    ("randstate_9x6_a2_v5_noovl", dict(width=9, height=6, num_agents=2, view_size=5, max_steps=12, allow_agent_overlap=False),
     48, 16, dict(density=0.3, terminated_p=0.3, carry_p=0.6)),
    ("randstate_10x8_a3_v7_all_joint", dict(width=10, height=8, num_agents=3, view_size=7, max_steps=14, joint_reward=True,
                                            success_termination_mode="all", failure_termination_mode="any"),
     48, 16, dict(density=0.35, terminated_p=0.15)),
    ("randstate_16x16_a4_v7", dict(width=16, height=16, num_agents=4, view_size=7, max_steps=20),
     32, 12, dict(density=0.3, terminated_p=0.15, carry_p=0.4)),
    ("randstate_13x10_a5_v9_noovl_any", dict(width=13, height=10, num_agents=5, view_size=9, max_steps=200, allow_agent_overlap=False,
                                             success_termination_mode="all", failure_termination_mode="any"),
     32, 14, dict(density=0.3, terminated_p=0.25, carry_p=0.5)),
    ("randstate_12x15_a7_v11_joint", dict(width=12, height=15, num_agents=7, view_size=11, max_steps=30, joint_reward=True),
     24, 12, dict(density=0.25, terminated_p=0.1)),
    ("randstate_20x14_a16_v15_noovl", dict(width=20, height=14, num_agents=16, view_size=15, max_steps=65535,
                                           allow_agent_overlap=False, failure_termination_mode="any"),
     16, 10, dict(density=0.2, terminated_p=0.2, carry_p=0.5)),
    ("randstate_10x9_a3_v7_boxes", dict(width=10, height=9, num_agents=3, view_size=7, max_steps=40),
     48, 16, dict(density=0.4, carry_p=0.5, box_contents_p=0.7)),
    ("randstate_10x8_a4_v5_edge", dict(width=10, height=8, num_agents=4, view_size=5, max_steps=30, allow_agent_overlap=False),
     32, 12, dict(density=0.3, terminated_p=0.1, edge_agents=True)),
    ("randstate_8x11_a2_v9_see_all", dict(width=8, height=11, num_agents=2, view_size=9, max_steps=1 << 20, see_through_walls=True,
                                          success_termination_mode="all", joint_reward=True),
     32, 14, dict(density=0.35, terminated_p=0.1, carry_p=0.4)),
    ("randstate_bup_11x6_a2_v7", dict(width=11, height=6, num_agents=2, view_size=7, max_steps=16, joint_reward=True,
                                      env_kind="blockedunlockpickup"),
     32, 16, dict(density=0.3, carry_p=0.5)),
    ("randstate_64x64_a16_v9", dict(width=64, height=64, num_agents=16, view_size=9, max_steps=4 * 64 * 64),
     16, 6, dict(density=0.08, terminated_p=0.1)),
]


def _bup_target(st, b, r):
    """BlockedUnlockPickup pays for carrying `env.obj` -- the one box object, by identity (envs/blockedunlockpickup.py:166-175,
    world_object.py: WorldObj.__eq__) -- while the product compares the carried cell with the target's bytes (aux).  A random state
    becomes a BlockedUnlockPickup state by keeping ONE box of the target's colour, in the grid or in an agent's hands, and giving the
    others another colour.  Returns where the target is: ("grid", x, y), ("agent", i) or None (no box left to be it)."""
    grid, agents = st["grid"][b], st["agents"][b]
    boxes = [("grid", int(x), int(y)) for y, x in np.argwhere(grid[..., 0] == 7)] + \
            [("agent", int(i)) for i in np.nonzero(agents[:, 5] == 7)[0]]
    where = boxes[int(r.integers(len(boxes)))] if boxes and r.random() < 0.9 else None
    if where is not None:
        c = int(grid[where[2], where[1], 1]) if where[0] == "grid" else int(agents[where[1], 6])
        st["target"][b, 1] = c
    c = int(st["target"][b, 1])
    for w in boxes:
        if w == where:
            continue
        cell = grid[w[2], w[1]] if w[0] == "grid" else agents[w[1], 5:8]
        if int(cell[1]) == c:
            cell[1] = (c + 1 + int(r.integers(5))) % 6
    return where


def _grey_walls_in_boxes(st):
    """Wall() is ONE cached instance in the reference (world_object.py:369-377: `functools.cache` on __new__), and
    WorldObj.decode writes the colour into it -- so a wall a box holds has the colour of the last wall decoded anywhere.  The
    reference's walls are grey; random_state's box contents give walls any colour: those are made grey here."""
    for arr in (st["grid"], st["agents"][..., 5:8]):
        code = arr[..., 2] >> 2
        wall = (arr[..., 0] == 7) & ((code & 7) == 6)
        arr[..., 2] = np.where(wall, (arr[..., 2] & 3) | ((6 | 5 << 3) << 2), arr[..., 2])


def _decode(t, c, s):
    """A product cell (type, color, state | content << 2) -> a reference WorldObj (or None), through WorldObj.decode."""
    from multigrid.core.world_object import WorldObj
    obj = WorldObj.decode(int(t), int(c), int(s) & 3 if t == 7 else int(s))
    if t == 7 and int(s) >> 2:
        code = int(s) >> 2
        kind, state = _CONTENT_CELL[code & 7]
        obj.contains = WorldObj.decode(kind, code >> 3, state)
    return obj


def _loaded_env(spec, st, b, target_at):
    """A reference env holding env `b` of the product-layout state `st`: a subclass of MultiGridEnv (or BlockedUnlockPickupEnv)
    whose _gen_grid -- the reference's extension point, base.py:229-247 -- builds Grid(W, H) with Grid.set and places the agents
    through their AgentState fields."""
    from multigrid.base import MultiGridEnv
    from multigrid.core.grid import Grid
    bup = spec["env_kind"] == "blockedunlockpickup"
    W, H, A = spec["width"], spec["height"], spec["num_agents"]
    grid, agents = st["grid"][b], st["agents"][b]

    def gen_grid(self, width, height):
        self.grid = Grid(width, height)
        self.obj = None
        for y in range(height):
            for x in range(width):
                t, c, s = (int(v) for v in grid[y, x])
                if t != 1:
                    obj = _decode(t, c, s)
                    self.grid.set(x, y, obj)
                    if target_at == ("grid", x, y):
                        self.obj = obj
        for agent in self.agents:
            row = agents[agent.index]
            agent.state.dir = int(row[1])
            agent.state.pos = (int(row[2]), int(row[3]))
            agent.state.terminated = bool(row[4])
            agent.state.carrying = _decode(*row[5:8]) if row[5] != 1 else None
            if target_at == ("agent", agent.index):
                self.obj = agent.state.carrying
        if bup and self.obj is None:                     # (the target box is nowhere: nothing can be paid for carrying it)
            self.obj = _decode(7, int(st["target"][b, 1]), 0)

    kw = dict(agents=A, max_steps=spec["max_steps"], agent_view_size=spec["view_size"], see_through_walls=spec["see_through_walls"],
              allow_agent_overlap=spec["allow_agent_overlap"], joint_reward=spec["joint_reward"],
              success_termination_mode=spec["success_termination_mode"], failure_termination_mode=spec["failure_termination_mode"])
    if bup:
        assert (W, H) == (11, 6)
        base = ref_envs.BlockedUnlockPickupEnv
        kw.pop("success_termination_mode")               # (BlockedUnlockPickupEnv fixes it to 'any')
        cls = type("LoadedBlockedUnlockPickup", (base,), dict(_gen_grid=gen_grid))
        env = cls(room_size=6, **kw)
    else:
        cls = type("LoadedState", (MultiGridEnv,), dict(_gen_grid=gen_grid))
        env = cls(width=W, height=H, **kw)
    env.reset(seed=0)
    lo_s, hi_s, lo_i, hi_i = (int(w) for w in st["rng"][b])
    bg = env.np_random.bit_generator
    state = bg.state
    state["state"] = {"state": lo_s | (hi_s << 64), "inc": lo_i | (hi_i << 64)}
    state["has_uint32"], state["uinteger"] = 0, 0
    bg.state = state
    env.step_count = int(st["step_count"][b])
    return env


def _product_rng(gen) -> np.ndarray:
    st = gen.bit_generator.state["state"]
    s, inc = int(st["state"]), int(st["inc"])
    return np.array([s & M64, s >> 64, inc & M64, inc >> 64], dtype=np.uint64)


def record_random_states():
    """Every spec of RANDSTATE_SPECS: a batch of tests.util.random_state envs, each loaded into the reference (_loaded_env) and
    stepped T times with random actions (5 % of the keys missing).  Arrays, all in the PRODUCT layout, batch-major per step:

        grid0 u8[B,H,W,3], agents0 u8[B,A,8], rng0 u64[B,4] ([state_lo, state_hi, inc_lo, inc_hi]), step_count0 i32[B], aux u8[B,16]
        obs0 u8[B,A,v,v,3], dir0 u8[B,A]                   env.gen_obs() of the loaded state
        actions i8[T,B,A]                                  -1 = the agent's key is absent from the dict
        obs u8[T,B,A,v,v,3], dir u8[T,B,A], reward f64[T,B,A], terminated u8[T,B,A], truncated u8[T,B]
        grid u8[T,B,H,W,3], agents u8[T,B,A,8], rng u64[T,B,4]   post-step state (box contents folded into the state bytes)
        spec_json                                          EnvSpec.as_dict() of the spec (+ the random_state keywords)"""
    sys.path.insert(0, REPO)
    from multigrid_amd import layouts
    from multigrid_amd.spec import EnvSpec
    from tests import util
    total = 0
    for n, (fname, kw, B, T, rs_kw) in enumerate(RANDSTATE_SPECS):
        spec = EnvSpec(**kw)
        sd = spec.as_dict()
        st = util.random_state(spec, B, seed=7000 + n, **rs_kw)
        _grey_walls_in_boxes(st)
        r = np.random.default_rng(8000 + n)
        if spec.env_kind == "blockedunlockpickup":
            targets = [_bup_target(st, b, r) for b in range(B)]
        else:
            targets = [None] * B
            st["target"][:] = 0
        # (forward-heavy, so that agents reach goals and lava, and run into each other)
        actions = r.choice(7, size=(T, B, spec.num_agents), p=[0.12, 0.12, 0.4, 0.1, 0.1, 0.12, 0.04]).astype(np.int8)
        actions[r.random(actions.shape) < 0.05] = -1
        rec = dict(grid0=st["grid"], agents0=st["agents"], rng0=st["rng"], step_count0=st["step_count"], aux=st["target"],
                   actions=actions)
        keys = ("obs", "dir", "reward", "terminated", "truncated", "grid", "agents", "rng")
        log = {k: [[None] * B for _ in range(T)] for k in keys}
        obs0, dir0 = [], []
        for b in range(B):
            env = _loaded_env(sd, st, b, targets[b])
            assert (layouts.grid_to_product(grid_with_contents(env)) == st["grid"][b]).all()
            assert (layouts.pack_agents(agents_with_contents(env)) == st["agents"][b]).all()
            o = env.gen_obs()
            obs0.append(np.stack([o[i]["image"] for i in range(spec.num_agents)]))
            dir0.append([int(o[i]["direction"]) for i in range(spec.num_agents)])
            for t in range(T):
                act = {i: int(a) for i, a in enumerate(actions[t, b]) if a >= 0}
                o, rew, term, trunc, _ = env.step(act)
                A = spec.num_agents
                log["obs"][t][b] = np.stack([o[i]["image"] for i in range(A)])
                log["dir"][t][b] = [int(o[i]["direction"]) for i in range(A)]
                log["reward"][t][b] = [float(rew[i]) for i in range(A)]
                log["terminated"][t][b] = [bool(term[i]) for i in range(A)]
                log["truncated"][t][b] = bool(trunc[0])
                log["grid"][t][b] = layouts.grid_to_product(grid_with_contents(env))
                log["agents"][t][b] = layouts.pack_agents(agents_with_contents(env))
                log["rng"][t][b] = _product_rng(env.np_random)
        rec["obs0"] = np.asarray(obs0).astype(np.uint8)
        rec["dir0"] = np.asarray(dir0).astype(np.uint8)
        for k in keys:
            arr = np.asarray(log[k])
            rec[k] = arr.astype(np.float64) if k == "reward" else arr if k == "rng" else arr.astype(np.uint8)
        rec["spec_json"] = np.array(json.dumps(dict(sd, random_state=rs_kw, seed=7000 + n)))
        path = os.path.join(OUT, fname + ".npz")
        np.savez_compressed(path, **rec)
        total += os.path.getsize(path)
        print(f"{fname:34s} B={B:3d} T={T:3d} success-steps={int((rec['reward'] > 0).any(axis=2).sum()):4d} "
              f"truncated={int(rec['truncated'].sum()):4d} {os.path.getsize(path) / 1024:.1f} KiB")
    print(f"random-state corpus: {total / 1024:.1f} KiB")
    assert total <= 1 << 20, "the random-state corpus must stay within 1 MiB"


# ---- the conflict corpus (tests/golden/conflict_*.npz): constructed envs in which the visiting order decides the outcome ----------
#: (file, EnvSpec keywords, boxes that hold something)
CONFLICT_SPECS = [
    ("conflict_9x6_a2_v5", dict(width=9, height=6, num_agents=2, view_size=5, max_steps=12, allow_agent_overlap=False,
                                failure_termination_mode="any"), False),
    ("conflict_16x16_a4_v7", dict(width=16, height=16, num_agents=4, view_size=7, max_steps=20), False),      # the C2 / C4 shape
    ("conflict_10x8_a3_v7", dict(width=10, height=8, num_agents=3, view_size=7, max_steps=14, allow_agent_overlap=False,
                                 joint_reward=True, success_termination_mode="all", failure_termination_mode="any"), False),
    ("conflict_13x10_a5_v9", dict(width=13, height=10, num_agents=5, view_size=9, max_steps=200, allow_agent_overlap=False,
                                  success_termination_mode="all"), False),
    ("conflict_20x14_a16_v9", dict(width=20, height=14, num_agents=16, view_size=9, max_steps=65535, joint_reward=True,
                                   failure_termination_mode="any"), False),
    ("conflict_bup_11x6_a2_v7", dict(width=11, height=6, num_agents=2, view_size=7, max_steps=16, joint_reward=True,
                                     env_kind="blockedunlockpickup"), False),
    ("conflict_10x8_a3_v7_boxes", dict(width=10, height=8, num_agents=3, view_size=7, max_steps=40), True),
    ("conflict_64x64_a16_v9", dict(width=64, height=64, num_agents=16, view_size=9, max_steps=4 * 64 * 64), False),   # the C5 shape
]
CONFLICT_INSTANCES = 8          # per scenario and file, before the batch is padded to its size

_E, _S, _W, _N = 0, 1, 2, 3     # agent directions (agent.py:111-118)
_LEFT, _FWD, _PICK, _DROP, _TOG = 0, 2, 3, 4, 5
_KEY, _BALL, _BOX, _GOAL, _LAVA = (5, 2, 0), (6, 1, 0), (7, 3, 0), (8, 1, 0), (9, 0, 0)
_BOX_KEY = (7, 3, (1 | 2 << 3) << 2)            # a box that holds a blue key / a floor tile (include/mgx.h "BOX CONTENTS")
_BOX_FLOOR = (7, 3, (4 | 0 << 3) << 2)
_OPEN, _CLOSED, _LOCKED = (4, 2, 0), (4, 2, 1), (4, 2, 2)
_BUP_TARGET = (7, 4, 0)                         # the one box BlockedUnlockPickup pays for; every other box above is purple


def _noovl(kw):
    return not kw.get("allow_agent_overlap", True)


#: The scenario table.  A scenario lives in a block of 4 x 2 cells; positions are (dx, dy) inside it.
#: (name, {cell: (type, colour, state)}, [(position, direction, carried cell or None, action)], admitted(spec keywords, boxes), event class)
#: event class: 0 none, 1 an event and a second agent with an effective action, 2 an event beside a cell conflict
#: Agents 0 and 1 of a row are the pair whose relative visiting order the recorder balances.
#: Not in the table, because the reference's outcome does not depend on the visiting order (the recorder's assertion fails on them):
#:   wrong key x forward              -- Door.toggle with another colour's key changes nothing, the forward is refused either way
#:   forward into a terminated agent  -- the terminated agent never moves, the forward is refused either way
#:   toggle x toggle on a closed door -- closed again in both orders; the row below is a LOCKED door and one matching key instead
#:   goal / lava under mode 'all' with agent overlap allowed -- the event ends only its own agent, nobody's inputs change; under
#:     'all' the event rows are the *_shared ones (two agents, one cell, no overlap)
CONFLICT_SCENARIOS = [
    # cell conflicts
    ("pickup_pickup", {(1, 0): _KEY}, [((0, 0), _E, None, _PICK), ((2, 0), _W, None, _PICK)], lambda kw, bx: True, 0),
    ("pickup_forward", {(1, 0): _KEY}, [((0, 0), _E, None, _PICK), ((2, 0), _W, None, _FWD)], lambda kw, bx: True, 0),
    ("drop_forward", {}, [((0, 0), _E, _BALL, _DROP), ((2, 0), _W, None, _FWD)], lambda kw, bx: True, 0),
    ("drop_drop", {}, [((0, 0), _E, _BALL, _DROP), ((2, 0), _W, _KEY, _DROP)], lambda kw, bx: True, 0),
    ("drop_pickup", {}, [((0, 0), _E, _BALL, _DROP), ((2, 0), _W, None, _PICK)], lambda kw, bx: True, 0),
    ("toggle_open_forward", {(1, 0): _OPEN}, [((0, 0), _E, None, _TOG), ((2, 0), _W, None, _FWD)], lambda kw, bx: True, 0),
    ("toggle_closed_forward", {(1, 0): _CLOSED}, [((0, 0), _E, None, _TOG), ((2, 0), _W, None, _FWD)], lambda kw, bx: True, 0),
    ("toggle_toggle", {(1, 0): _LOCKED}, [((0, 0), _E, _KEY, _TOG), ((2, 0), _W, None, _TOG)], lambda kw, bx: True, 0),
    ("unlock_forward", {(1, 0): _LOCKED}, [((0, 0), _E, _KEY, _TOG), ((2, 0), _W, None, _FWD)], lambda kw, bx: True, 0),
    ("togglebox_pickup", {(1, 0): _BOX}, [((0, 0), _E, None, _TOG), ((2, 0), _W, None, _PICK)], lambda kw, bx: True, 0),
    ("togglebox_forward", {(1, 0): _BOX}, [((0, 0), _E, None, _TOG), ((2, 0), _W, None, _FWD)], lambda kw, bx: True, 0),
    ("togglefilled_pickup", {(1, 0): _BOX_KEY}, [((0, 0), _E, None, _TOG), ((2, 0), _W, None, _PICK)], lambda kw, bx: bx, 0),
    ("togglefilled_forward", {(1, 0): _BOX_FLOOR}, [((0, 0), _E, None, _TOG), ((2, 0), _W, None, _FWD)], lambda kw, bx: bx, 0),
    ("pickupfilled_pickup", {(1, 0): _BOX_KEY}, [((0, 0), _E, None, _PICK), ((2, 0), _W, None, _PICK)], lambda kw, bx: bx, 0),
    ("pickup_pickup_target", {(1, 0): _BUP_TARGET}, [((0, 0), _E, None, _PICK), ((2, 0), _W, None, _PICK)],
     lambda kw, bx: kw.get("env_kind") == "blockedunlockpickup", 0),
    # presence
    ("forward_forward_one_cell", {}, [((0, 0), _E, None, _FWD), ((2, 0), _W, None, _FWD)], lambda kw, bx: _noovl(kw), 0),
    ("forward_into_vacated", {}, [((0, 0), _E, None, _FWD), ((1, 0), _E, None, _FWD)], lambda kw, bx: _noovl(kw), 0),
    ("line_of_three", {}, [((0, 0), _E, None, _FWD), ((1, 0), _E, None, _FWD), ((2, 0), _E, None, _FWD)],
     lambda kw, bx: _noovl(kw), 0),
    ("drop_before_arriving", {}, [((0, 0), _E, _BALL, _DROP), ((1, 1), _N, None, _FWD)], lambda kw, bx: True, 0),
    ("drop_behind_leaving", {}, [((0, 0), _E, _BALL, _DROP), ((1, 0), _E, None, _FWD)], lambda kw, bx: True, 0),
    # events: the second agent holds an effective action
    ("goal_other_acts", {(1, 0): _GOAL}, [((0, 0), _E, None, _FWD), ((0, 1), _E, None, _FWD)],
     lambda kw, bx: kw.get("success_termination_mode", "any") == "any", 1),
    ("lava_other_acts", {(1, 0): _LAVA}, [((0, 0), _E, None, _FWD), ((0, 1), _E, None, _FWD)],
     lambda kw, bx: kw.get("failure_termination_mode", "all") == "any", 1),
    ("goal_shared", {(1, 0): _GOAL}, [((0, 0), _E, None, _FWD), ((2, 0), _W, None, _FWD)], lambda kw, bx: _noovl(kw), 1),
    ("lava_shared", {(1, 0): _LAVA}, [((0, 0), _E, None, _FWD), ((2, 0), _W, None, _FWD)], lambda kw, bx: _noovl(kw), 1),
    # ... inside an env that also has a cell conflict: the event is the sequential loop's
    ("goal_beside_conflict", {(1, 0): _KEY, (1, 1): _GOAL},
     [((0, 0), _E, None, _PICK), ((2, 0), _W, None, _FWD), ((0, 1), _E, None, _FWD)], lambda kw, bx: True, 2),
    ("lava_beside_conflict", {(1, 0): _KEY, (1, 1): _LAVA},
     [((0, 0), _E, None, _PICK), ((2, 0), _W, None, _FWD), ((0, 1), _E, None, _FWD)], lambda kw, bx: True, 2),
]


def _order_of(words, A):
    """The visiting order handle_actions draws (base.py:396-399) from the generator state `words` (product order)."""
    bg = np.random.PCG64()
    st = bg.state
    st["state"] = {"state": int(words[0]) | (int(words[1]) << 64), "inc": int(words[2]) | (int(words[3]) << 64)}
    st["has_uint32"], st["uinteger"] = 0, 0
    bg.state = st
    return np.random.Generator(bg).random(size=A).argsort()


def _conflict_batch(kw, boxes):
    """The envs of one file: lists of (scenario row, instance number) packed into the spec's A agents, events in envs of their own
    (an ends-all event would blur the other scenarios' own order dependence); then padded until the batch is odd and no multiple
    of any number of envs a wavefront can hold (one lane per agent: at most 64 // A)."""
    A, W, H = kw["num_agents"], kw["width"], kw["height"]
    rows = [sc for sc in CONFLICT_SCENARIOS if sc[3](kw, boxes) and len(sc[2]) <= A]
    envs = []

    def pack(instances, most):
        cur, used = [], 0
        for sc, k in instances:
            n = len(sc[2])
            if used + n > A or len(cur) == most:
                envs.append(cur)
                cur, used = [], 0
            cur.append((sc, k))
            used += n
        if cur:
            envs.append(cur)

    pack([(sc, k) for k in range(CONFLICT_INSTANCES) for sc in rows if sc[4] == 0], 8)
    # an event alone in its env, three times as often: only where nothing else forces the sequential loop does the EVENT CUTOFF of
    # the order-free path decide who acts, and only in half of the orders does it suppress anybody
    pack([(sc, k) for k in range(3 * CONFLICT_INSTANCES) for sc in rows if sc[4] == 1], 1)
    pack([(sc, k) for k in range(CONFLICT_INSTANCES) for sc in rows if sc[4] == 2], 2)
    k = CONFLICT_INSTANCES
    while len(envs) % 2 == 0 or any(len(envs) % g == 0 for g in range(2, 64 // A + 1)):
        n0 = len(envs)
        pack([(sc, k) for sc in rows], 8)
        del envs[n0 + 1:]
        k += 1
    return rows, envs


def record_conflicts():
    """Every spec of CONFLICT_SPECS: envs BUILT so that the visiting order decides the outcome -- every row of CONFLICT_SCENARIOS the
    spec admits, CONFLICT_INSTANCES times, from generator states chosen so that the row's first two agents are visited in either
    order -- each loaded into the reference (_loaded_env) and stepped twice with the row's actions.  The recorder ASSERTS, per file
    and row, that two distinct visiting orders occurred and that the reference's post-step state or outputs differ between them.

    Arrays: exactly those of record_random_states, and
        order u8[T,B,A]        the visiting order of each step         scenario str[B]    the rows an env holds, '+'-joined
        cluster_agents i8[B,8,3], cluster_block u8[B,8,2]   per env and cluster: its agents (-1 = none), its block's (x, y)"""
    sys.path.insert(0, REPO)
    from multigrid_amd import layouts
    from multigrid_amd.spec import EnvSpec
    total = 0
    T = 2
    for n, (fname, kw, boxes) in enumerate(CONFLICT_SPECS):
        spec = EnvSpec(**kw)
        sd = spec.as_dict()
        A, W, H = spec.num_agents, spec.width, spec.height
        bup = spec.env_kind == "blockedunlockpickup"
        rows_admitted, envs = _conflict_batch(kw, boxes)
        B = len(envs)
        assert B % 2 == 1 and all(B % g for g in range(2, 64 // A + 1)), B
        across = (W - 2) // 4
        r = np.random.default_rng(9000 + n)
        grid = np.zeros((B, H, W, 3), np.uint8)
        grid[..., 0] = 1
        grid[:, 0, :] = grid[:, -1, :] = grid[:, :, 0] = grid[:, :, -1] = (2, 5, 0)
        agents = np.zeros((B, A, 8), np.uint8)
        agents[..., 0] = np.arange(A) % 6
        agents[..., 5] = 1
        rng = np.zeros((B, 4), np.uint64)
        actions = np.zeros((T, B, A), np.int8)
        cl_agents = np.full((B, 8, 3), -1, np.int8)
        cl_block = np.zeros((B, 8, 2), np.uint8)
        aux = np.zeros((B, 16), np.uint8)
        targets = [None] * B
        step_count = (np.arange(B) % max(1, spec.max_steps - T)).astype(np.int32)
        for b, env in enumerate(envs):
            a, want = 0, []
            for c, (sc, k) in enumerate(env):
                bx, by = 1 + 4 * (c % across), 1 + 2 * (c // across)
                cl_block[b, c] = bx, by
                for (dx, dy), cell in sc[1].items():
                    grid[b, by + dy, bx + dx] = cell
                    if cell == _BUP_TARGET:
                        targets[b] = ("grid", bx + dx, by + dy)
                for j, ((dx, dy), d, carry, action) in enumerate(sc[2]):
                    agents[b, a, 1:4] = d, bx + dx, by + dy
                    agents[b, a, 5:8] = carry if carry is not None else (1, 0, 0)
                    actions[:, b, a] = action
                    cl_agents[b, c, j] = a
                    a += 1
                i0 = a - len(sc[2])
                want.append((i0, i0 + 1, bool(k & 1)))
                if sc[4] == 2:                           # the event's agent ahead of the conflicting pair, or behind one of them
                    want.append((i0 + 2, i0 if k & 1 else i0 + 1, bool(k & 2)))
            c = len(env)
            for j in range(A - a):                       # the agents no row uses turn on the spot, in blocks of their own
                cj = c + j // 8
                agents[b, a + j, 1:4] = _N, 1 + 4 * (cj % across) + j % 4, 1 + 2 * (cj // across) + j % 8 // 4
                actions[:, b, a + j] = _LEFT
            assert len(env) <= 8 and c + (A - a + 7) // 8 <= across * ((H - 2) // 2), "the grid has too few blocks"
            if bup:
                aux[b, :3] = _BUP_TARGET
            while True:                                      # a generator state under which every pair is visited as wanted
                w = r.integers(0, 2 ** 63, size=4, dtype=np.int64).astype(np.uint64)
                w[2] |= np.uint64(1)
                rank = np.argsort(_order_of(w, A))
                if all((rank[i] < rank[j]) == first for i, j, first in want):
                    break
            rng[b] = w
        st = dict(grid=grid, agents=agents, rng=rng, step_count=step_count, target=aux)
        rec = dict(grid0=grid, agents0=agents, rng0=rng, step_count0=step_count, aux=aux, actions=actions,
                   cluster_agents=cl_agents, cluster_block=cl_block,
                   scenario=np.array(["+".join(sc[0] for sc, _ in env) for env in envs]))
        keys = ("obs", "dir", "reward", "terminated", "truncated", "grid", "agents", "rng", "order")
        log = {k: [[None] * B for _ in range(T)] for k in keys}
        obs0, dir0 = [], []
        for b in range(B):
            env = _loaded_env(sd, st, b, targets[b])
            assert (layouts.grid_to_product(grid_with_contents(env)) == grid[b]).all()
            assert (layouts.pack_agents(agents_with_contents(env)) == agents[b]).all()
            o = env.gen_obs()
            obs0.append(np.stack([o[i]["image"] for i in range(A)]))
            dir0.append([int(o[i]["direction"]) for i in range(A)])
            for t in range(T):
                log["order"][t][b] = clone_order(env.np_random, A)
                o, rew, term, trunc, _ = env.step({i: int(x) for i, x in enumerate(actions[t, b])})
                log["obs"][t][b] = np.stack([o[i]["image"] for i in range(A)])
                log["dir"][t][b] = [int(o[i]["direction"]) for i in range(A)]
                log["reward"][t][b] = [float(rew[i]) for i in range(A)]
                log["terminated"][t][b] = [bool(term[i]) for i in range(A)]
                log["truncated"][t][b] = bool(trunc[0])
                log["grid"][t][b] = layouts.grid_to_product(grid_with_contents(env))
                log["agents"][t][b] = layouts.pack_agents(agents_with_contents(env))
                log["rng"][t][b] = _product_rng(env.np_random)
            assert (log["order"][0][b] == _order_of(rng[b], A)).all()
        rec["obs0"] = np.asarray(obs0).astype(np.uint8)
        rec["dir0"] = np.asarray(dir0).astype(np.uint8)
        for k in keys:
            arr = np.asarray(log[k])
            rec[k] = arr.astype(np.float64) if k == "reward" else arr if k == "rng" else arr.astype(np.uint8)
        # order sensitivity, row by row: the first step's outcome INSIDE the cluster (its agents' rows without the colour byte, its
        # block's cells, who was paid, who is terminated), keyed by the relative visiting order of the cluster's agents
        for sc in rows_admitted:
            seen = {}
            for b, env in enumerate(envs):
                if not sc[4] and any(other[4] for other, _ in env):
                    continue                             # (a padding env that mixes this row with an event)
                for c, (other, _) in enumerate(env):
                    if other is not sc:
                        continue
                    ag = [int(i) for i in cl_agents[b, c] if i >= 0]
                    rank = np.argsort(rec["order"][0, b])
                    key = tuple(np.argsort([rank[i] for i in ag]))
                    bx, by = (int(v) for v in cl_block[b, c])
                    out = (rec["agents"][0, b, ag, 1:].tobytes(), rec["grid"][0, b, by:by + 2, bx:bx + 4].tobytes(),
                           (rec["reward"][0, b, ag] > 0).tobytes(), rec["terminated"][0, b, ag].tobytes())
                    seen.setdefault(key, set()).add(out)
            assert len(seen) >= 2, f"{fname} {sc[0]}: one visiting order only"
            outs = list(seen.values())
            assert any(x != y for i, x in enumerate(outs) for y in outs[i + 1:]), \
                f"{fname} {sc[0]}: the reference's outcome does not depend on the visiting order"
        rec["spec_json"] = np.array(json.dumps(dict(sd, conflict_rows=[sc[0] for sc in rows_admitted], seed=9000 + n)))
        path = os.path.join(OUT, fname + ".npz")
        np.savez_compressed(path, **rec)
        total += os.path.getsize(path)
        print(f"{fname:30s} B={B:3d} T={T} rows={len(rows_admitted):2d} success-steps={int((rec['reward'] > 0).any(axis=2).sum()):4d} "
              f"{os.path.getsize(path) / 1024:.1f} KiB")
    print(f"conflict corpus: {total / 1024:.1f} KiB")
    assert total <= 512 << 10, "the conflict corpus must stay within 512 KiB"


# ---- the reset corpus (tests/golden/resets_*.npz): single resets of the REAL reference from given generator states ---------------
#: (file tag, generator kind of the product, reference class name, constructor keywords, events)
RESET_CONFIGS = [
    ("empty_random_4_a3_full", "empty_random", "EmptyEnv", dict(size=4, agents=3, agent_view_size=3, agent_start_pos=None), 12),
    ("empty_random_5_a8_full", "empty_random", "EmptyEnv", dict(size=5, agents=8, agent_view_size=3, agent_start_pos=None), 8),
    ("empty_random_6_a3", "empty_random", "EmptyEnv", dict(size=6, agents=3, agent_view_size=5, agent_start_pos=None), 12),
    ("empty_random_9_a4", "empty_random", "EmptyEnv", dict(size=9, agents=4, agent_start_pos=None), 12),
    ("empty_random_16_a5", "empty_random", "EmptyEnv", dict(size=16, agents=5, agent_start_pos=None), 12),
    ("empty_fixed_8_a2", "empty_fixed", "EmptyEnv", dict(size=8, agents=2), 4),
    ("empty_fixed_5_a3", "empty_fixed", "EmptyEnv", dict(size=5, agents=3, agent_view_size=3, agent_start_pos=(2, 3), agent_start_dir=1), 4),
    ("bup_rs4_a2_full", "blockedunlockpickup", "BlockedUnlockPickupEnv", dict(room_size=4, agents=2, agent_view_size=3), 12),
    ("bup_rs5_a7_full", "blockedunlockpickup", "BlockedUnlockPickupEnv", dict(room_size=5, agents=7, agent_view_size=3), 8),
    ("bup_rs5_a2", "blockedunlockpickup", "BlockedUnlockPickupEnv", dict(room_size=5, agents=2, agent_view_size=5), 12),
    ("bup_rs6_a3", "blockedunlockpickup", "BlockedUnlockPickupEnv", dict(room_size=6, agents=3), 16),
    ("bup_rs7_a2", "blockedunlockpickup", "BlockedUnlockPickupEnv", dict(room_size=7, agents=2), 12),
    ("bup_rs8_a4", "blockedunlockpickup", "BlockedUnlockPickupEnv", dict(room_size=8, agents=4), 12),
    ("bup_rs9_a2", "blockedunlockpickup", "BlockedUnlockPickupEnv", dict(room_size=9, agents=2), 12),
    ("rbd_4_a4_full", "redbluedoors", "RedBlueDoorsEnv", dict(size=4, agents=4, agent_view_size=3), 12),
    ("rbd_5_a2", "redbluedoors", "RedBlueDoorsEnv", dict(size=5, agents=2, agent_view_size=5), 12),
    ("rbd_6_a3", "redbluedoors", "RedBlueDoorsEnv", dict(size=6, agents=3, agent_view_size=5), 12),
    ("rbd_8_a3", "redbluedoors", "RedBlueDoorsEnv", dict(size=8, agents=3), 12),
    ("rbd_12_a4", "redbluedoors", "RedBlueDoorsEnv", dict(size=12, agents=4), 12),
    ("lh_2rooms_rs4_k11_a3_full", "lockedhallway", "LockedHallwayEnv",
     dict(num_rooms=2, room_size=4, max_hallway_keys=1, max_keys_per_room=1, agents=3, agent_view_size=3), 12),
    ("lh_2rooms_rs5_k33_a2", "lockedhallway", "LockedHallwayEnv",
     dict(num_rooms=2, room_size=5, max_hallway_keys=3, max_keys_per_room=3, agents=2, agent_view_size=5), 12),
    ("lh_4rooms_rs5_k12_a2", "lockedhallway", "LockedHallwayEnv",
     dict(num_rooms=4, room_size=5, max_hallway_keys=1, max_keys_per_room=2, agents=2), 12),
    ("lh_4rooms_rs4_k22_a2", "lockedhallway", "LockedHallwayEnv",
     dict(num_rooms=4, room_size=4, max_hallway_keys=2, max_keys_per_room=2, agents=2, agent_view_size=5), 12),
    ("lh_6rooms_rs5_k23_a3", "lockedhallway", "LockedHallwayEnv",
     dict(num_rooms=6, room_size=5, max_hallway_keys=2, max_keys_per_room=3, agents=3), 12),
    ("lh_8rooms_rs6_k23_a3", "lockedhallway", "LockedHallwayEnv",
     dict(num_rooms=8, room_size=6, max_hallway_keys=2, max_keys_per_room=3, agents=3), 12),
    ("lh_12rooms_rs4_k31_a2", "lockedhallway", "LockedHallwayEnv",
     dict(num_rooms=12, room_size=4, max_hallway_keys=3, max_keys_per_room=1, agents=2, agent_view_size=5), 12),
    ("lh_16rooms_rs7_k33_a4", "lockedhallway", "LockedHallwayEnv",
     dict(num_rooms=16, room_size=7, max_hallway_keys=3, max_keys_per_room=3, agents=4), 8),
    ("playground_1x1_rs7_a1", "playground", "PlaygroundEnv", dict(num_rows=1, num_cols=1, room_size=7, agents=1), 8),
    ("playground_1x2_rs7_a2", "playground", "PlaygroundEnv", dict(num_rows=1, num_cols=2, room_size=7, agents=2), 12),
    ("playground_2x3_rs6_a2", "playground", "PlaygroundEnv", dict(num_rows=2, num_cols=3, room_size=6, agents=2, agent_view_size=5), 12),
    ("playground_3x3_rs7_a3", "playground", "PlaygroundEnv", dict(num_rows=3, num_cols=3, room_size=7, agents=3), 12),
    ("playground_3x4_rs8_a1", "playground", "PlaygroundEnv", dict(num_rows=3, num_cols=4, room_size=8, agents=1), 8),
    ("playground_4x4_rs6_a3", "playground", "PlaygroundEnv", dict(num_rows=4, num_cols=4, room_size=6, agents=3), 8),
]
#: the configurations whose pre-states are CONSTRUCTED so that a bounded draw re-samples (one per generator kind that draws)
RESET_CONSTRUCTED = ["empty_random_6_a3", "bup_rs6_a3", "bup_rs7_a2", "rbd_6_a3", "lh_6rooms_rs5_k23_a3", "playground_2x3_rs6_a2"]
_PCG_MULT = 0x2360ED051FC65DA44385DF649FCCF645
_PCG_INV = pow(_PCG_MULT, -1, 1 << 128)
_M128 = (1 << 128) - 1


def _pcg_out(s):
    hi, lo = s >> 64, s & M64
    rot, x = hi >> 58, hi ^ lo
    return ((x >> rot) | (x << ((64 - rot) & 63))) & M64


def _gen_words5(gen):
    st = gen.bit_generator.state
    s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
    return np.array([s & M64, s >> 64, inc & M64, inc >> 64, (int(st["has_uint32"]) << 32) | int(st["uinteger"])], dtype=np.uint64)


def _halves_between(before, after):
    """32-bit draws made between two bit-generator states of one stream (position = 2 * words made - has_uint32)."""
    s, inc, target = int(before["state"]["state"]), int(before["state"]["inc"]), int(after["state"]["state"])
    words = 0
    while s != target:
        s = (s * _PCG_MULT + inc) & _M128
        words += 1
        assert words < 1 << 20
    return 2 * words - int(after["has_uint32"]) + int(before["has_uint32"])


def _half_stream(state, n):
    """The next n 32-bit draws of a bit-generator state (numpy's next_uint32: the low half of a word, then its buffered high half)."""
    s, inc = int(state["state"]["state"]), int(state["state"]["inc"])
    out = [int(state["uinteger"])] if state["has_uint32"] else []
    while len(out) < n:
        s = (s * _PCG_MULT + inc) & _M128
        w = _pcg_out(s)
        out += [w & 0xFFFFFFFF, w >> 32]
    return out[:n]


def _lemire_rejects(half, span):
    """Would Generator.integers over `span` values re-sample on this 32-bit draw?  (numpy's distributions.c, buffered_bounded_lemire_uint32)"""
    return ((half * span) & 0xFFFFFFFF) < ((1 << 32) - span) % span


def _constructed_state(base, k, high, salt):
    """`base` (a bit-generator state dict) with its 128-bit state replaced so that word k from here (0 = the next one made) has a zero
    low / high half: a next state with hi >> 58 == 0 (no rotation) and lo = hi ^ out, stepped back k + 1 times."""
    inc = int(base["state"]["inc"])
    r = np.random.default_rng([0x5E7, k, int(high), salt])
    hi = int(r.integers(0, 1 << 58))
    other = int(r.integers(1, 1 << 32))
    out = other if high else other << 32
    s = (hi << 64) | (hi ^ out)
    for _ in range(k + 1):
        s = ((s - inc) * _PCG_INV) & _M128
    st = dict(base)
    st["state"] = dict(state=s, inc=inc)
    return st


class _ResetProbe:
    """Instrumentation from outside: wraps RandomMixin._rand_int / _rand_perm, MultiGridEnv.place_obj and RoomGrid.add_object of the
    reference while a reset runs, and logs what the placement generator was asked for."""

    def __init__(self):
        from multigrid.base import MultiGridEnv
        from multigrid.core.roomgrid import RoomGrid
        from multigrid.utils.random import RandomMixin
        self.targets = [(RandomMixin, "_rand_int"), (RandomMixin, "_rand_perm"), (MultiGridEnv, "place_obj"), (RoomGrid, "add_object")]
        self.saved = [getattr(c, n) for c, n in self.targets]
        self.clear()

    def clear(self):
        self.draws, self.calls, self.shuffles, self.rooms, self.in_call = [], [], [], [], None

    def __enter__(self):
        probe, (rand_int, rand_perm, place_obj, add_object) = self, self.saved

        def _rand_int(env, low, high):
            g = env._RandomMixin__np_random.bit_generator
            before = g.state
            v = rand_int(env, low, high)
            span = int(high) - int(low)
            n = _halves_between(before, g.state)
            assert n == (span > 1) or (span > 1 and n > 1)
            probe.draws.append(dict(lo=int(low), hi=int(high), value=int(v), halves=n, pending=int(before["has_uint32"]),
                                    call=probe.in_call, before=before))
            return v

        def _rand_perm(env, iterable):
            g = env._RandomMixin__np_random.bit_generator
            before = g.state
            out = rand_perm(env, iterable)
            probe.shuffles.append(dict(n=len(out), halves=_halves_between(before, g.state), pending=int(before["has_uint32"])))
            return out

        def _place_obj(env, obj, top=None, size=None, reject_fn=None, max_tries=float("inf")):
            assert probe.in_call is None
            probe.in_call = len(probe.calls)
            first = len(probe.draws)
            before = env._RandomMixin__np_random.bit_generator.state
            try:
                return place_obj(env, obj, top, size, reject_fn, max_tries)
            finally:
                probe.calls.append(dict(first=first, ndraws=len(probe.draws) - first, before=before))
                probe.in_call = None

        def _add_object(env, col, row, kind=None, color=None):
            probe.rooms.append(int(row) * env.num_cols + int(col))
            return add_object(env, col, row, kind, color)

        for (c, n), f in zip(self.targets, (_rand_int, _rand_perm, _place_obj, _add_object)):
            setattr(c, n, f)
        return self

    def __exit__(self, *exc):
        for (c, n), f in zip(self.targets, self.saved):
            setattr(c, n, f)


def _reset_event(env, probe, lay_state, npr_state, bup):
    """One unseeded reset() of `env` from the two given bit-generator states -> (arrays, instrumentation rows)."""
    lay, npr = env._RandomMixin__np_random, env.np_random
    assert lay is not npr
    lay.bit_generator.state, npr.bit_generator.state = lay_state, npr_state
    A = env.num_agents
    ev = dict(lay_before=_gen_words5(lay), npr_before=_gen_words5(npr))
    probe.clear()
    obs, _ = env.reset()
    assert env._RandomMixin__np_random is lay and env.np_random is npr
    ev.update(grid0=layouts_mod.grid_to_product(grid_with_contents(env)), agents0=layouts_mod.pack_agents(agents_with_contents(env)),
              obs0=np.stack([obs[i]["image"] for i in range(A)]).astype(np.uint8), lay_after=_gen_words5(lay), npr_after=_gen_words5(npr),
              lay_halves=_halves_between(lay_state, lay.bit_generator.state), npr_halves=_halves_between(npr_state, npr.bit_generator.state))
    if bup:
        ev["target"] = np.array([int(v) for v in np.asarray(env.obj)], dtype=np.uint8)
    # call rows: [tries, x span, y span, real re-samples inside the call, a later try of the first fit's group of eight claims one]
    calls, resamples = [], []
    for ci, c in enumerate(probe.calls):
        d = probe.draws[c["first"]:c["first"] + c["ndraws"]]
        assert len(d) % 2 == 0 and len(d) >= 2
        tries, xs, ys = len(d) // 2, d[0]["hi"] - d[0]["lo"], d[1]["hi"] - d[1]["lo"]
        real = 0
        for k, dr in enumerate(d):
            if dr["halves"] > 1:
                real += 1          # [generator, call, try, half of the rejected draw (1 = a pending high half), inside a call]
                resamples.append([0, ci, k // 2, (dr["pending"] + 0) & 1, 1])
        later = 0
        if xs >= 2 and ys >= 2 and real == 0:
            # what the lanes behind the fitting try of a group of eight would see: tries f + 1 .. 7 of that round, read as (x, y) draws
            f = (tries - 1) % 8
            hs = _half_stream(c["before"], 2 * (tries - 1 - f + 8))[2 * (tries - 1 - f):]
            later = int(any(_lemire_rejects(hs[2 * j], xs) or _lemire_rejects(hs[2 * j + 1], ys) for j in range(f + 1, 8)))
        calls.append([tries, xs, ys, real, later])
    for dr in probe.draws:
        if dr["call"] is None and dr["halves"] > 1:
            resamples.append([0, -1, -1, dr["pending"] & 1, 0])
    if bup and ev["npr_halves"] > 1:
        resamples.append([1, -1, -1, int(npr_state["has_uint32"]) & 1, 0])
    info = dict(calls=calls, resamples=resamples,
                shuffles=[[s["n"], s["halves"] - (s["n"] - 1), s["pending"]] for s in probe.shuffles],
                key_draws=[[dr["hi"] - 1, dr["value"]] for dr in probe.draws if dr["call"] is None and dr["lo"] == 1],
                rooms=list(probe.rooms))
    return ev, info


def _reset_pre_states(tag, i):
    """Event i's generator states: seeded PCG64 streams a few draws in; (i & 1, i & 2) = a pending 32-bit half on (placement, np_random)."""
    out = []
    for which in (0, 1):
        g = np.random.Generator(np.random.PCG64([0x2E5E7, which, i] + [ord(c) for c in tag]))
        g.random(i % 3)
        if (i >> which) & 1:
            g.integers(0, 5)
            assert g.bit_generator.state["has_uint32"] == 1
        out.append(g.bit_generator.state)
    return out


def _write_resets(fname, env, kind, kw, events, infos):
    rec = {k: np.stack([e[k] for e in events]) for k in events[0] if k not in ("lay_halves", "npr_halves")}
    for k in ("grid0", "agents0", "obs0"):
        rec[k] = rec[k].astype(np.uint8)
    rec["lay_halves"] = np.array([e["lay_halves"] for e in events], dtype=np.int32)
    rec["npr_halves"] = np.array([e["npr_halves"] for e in events], dtype=np.int32)
    for name, width in (("calls", 5), ("resamples", 5), ("shuffles", 3), ("key_draws", 2)):
        rows = [[n] + list(r) for n, info in enumerate(infos) for r in info[name]]
        rec[name] = np.asarray(rows, dtype=np.int32).reshape(-1, width + 1)
    if kind == "playground":
        rec["object_rooms"] = narrow(np.asarray([info["rooms"] for info in infos]))
    gen = dict(kind=kind, room_size=int(kw.get("room_size", 0)), max_hallway_keys=int(kw.get("max_hallway_keys", 1)),
               max_keys_per_room=int(kw.get("max_keys_per_room", 2)),
               start=[int(v) for v in (*(kw.get("agent_start_pos", (1, 1)) or (1, 1)), kw.get("agent_start_dir", 0))])
    env_kind = kind if kind in ("blockedunlockpickup", "redbluedoors", "lockedhallway") else "empty"
    rec["spec_json"] = np.array(json.dumps(dict(spec_of_noreset(env, env_kind), gen=gen)))
    path = os.path.join(OUT, fname + ".npz")
    np.savez_compressed(path, **rec)
    c = rec["calls"]
    print(f"{fname:40s} events={len(events):3d} calls={len(c):4d} max tries={int(c[:, 1].max()) if len(c) else 0:3d} "
          f"re-samples={len(rec['resamples']):2d} pending(lay,npr)={int((rec['lay_before'][:, 4] >> np.uint64(32)).sum())},"
          f"{int((rec['npr_before'][:, 4] >> np.uint64(32)).sum())} {os.path.getsize(path) / 1024:.1f} KiB")
    return os.path.getsize(path)


def record_resets():
    """The reset corpus: every file holds N independent unseeded reset() calls of ONE generator configuration of the real reference,
    each from given states of its two generators (the placement generator `_RandomMixin__np_random` and `env.np_random`).  Arrays
    (product layout; generator states as u64[5] = [state_lo, state_hi, inc_lo, inc_hi, has_uint32 << 32 | uinteger]):

        lay_before, npr_before u64[N,5]      the two generators just before reset()
        grid0 u8[N,H,W,3], agents0 u8[N,A,8], obs0 u8[N,A,v,v,3], target u8[N,3] (BlockedUnlockPickup: env.obj)
        lay_after, npr_after u64[N,5]        the states the reset left
        lay_halves, npr_halves i32[N]        32-bit draws each generator made
        calls i32[M,6]       per place_obj call: [event, tries, x span, y span, re-samples inside the call, a LATER try of the fitting
                             try's group of eight -- read as an (x, y) draw -- would claim a re-sample (what the group must ignore).
                             This last column is COMPUTED by the recorder (_half_stream, _lemire_rejects: its own PCG64 and Lemire
                             threshold over draws the reference never made), not observed; the re-samples the same model predicts
                             inside a call are checked against the observed ones]
        resamples i32[R,6]   per bounded draw that re-sampled: [event, generator (0 placement / 1 np_random), place_obj call (-1:
                             outside), try, rejected draw was a pending high half, inside a place_obj call (= before its first fit)]
        shuffles i32[S,4]    per Generator.shuffle (_rand_perm): [event, n, rejected masked draws, started on a pending half]
        key_draws i32[K,3]   LockedHallway's key counts: [event, maximum, drawn]
        object_rooms [N,12]  Playground: the room (row * cols + col) each of the 12 objects drew
        spec_json            EnvSpec fields + "gen": the keywords of set_layout_generator

    resets_con_*: the same configuration from CONSTRUCTED placement (and np_random) states whose word k has a zero low / high half,
    so that a bounded draw over a span that is no power of two re-samples there; kept when the instrumentation shows an event of
    a kind the file does not hold three of yet."""
    global layouts_mod
    sys.path.insert(0, REPO)
    from multigrid_amd import layouts as layouts_mod
    total = 0
    with _ResetProbe() as probe:
        for n, (tag, kind, cls_name, kw, N) in enumerate(RESET_CONFIGS):
            cls = getattr(ref_envs, cls_name)
            cls._default_seed = 0x5E7000 + n
            env = cls(**kw)
            env.reset(seed=n)
            bup = kind == "blockedunlockpickup"
            events, infos = [], []
            for i in range(N):
                ev, info = _reset_event(env, probe, *_reset_pre_states(tag, i), bup)
                events.append(ev); infos.append(info)
            total += _write_resets("resets_" + tag, env, kind, kw, events, infos)
            if tag not in RESET_CONSTRUCTED:
                continue
            events, infos, have = [], [], {}
            for k in range(41):
                for high in (0, 1):
                    for pend in (0, 1):
                        lay_state, npr_state = _reset_pre_states(tag, 3 * pend)      # (event 3: a pending half on both generators)
                        lay_state = _constructed_state(lay_state, k, high, n)
                        if bup and k < 4:                                             # np_random's one draw: the door row
                            npr_state = _constructed_state(npr_state, 0, high, n) if not pend else dict(npr_state, has_uint32=1, uinteger=0)
                        ev, info = _reset_event(env, probe, lay_state, npr_state, bup)
                        kinds = set()
                        for r in info["resamples"]:
                            kinds.add(("npr",) if r[0] == 1 else ("lay", r[3], r[4]))
                        for c in info["calls"]:
                            if c[4]:
                                kinds.add(("later",))
                            if c[3] and c[0] > 8:
                                kinds.add(("second round",))
                        new = [q for q in kinds if have.get(q, 0) < 3]
                        if new:
                            for q in kinds:
                                have[q] = have.get(q, 0) + 1
                            events.append(ev); infos.append(info)
            total += _write_resets("resets_con_" + tag, env, kind, kw, events, infos)
    print(f"reset corpus: {total / 1024:.1f} KiB")
    assert total <= 800 << 10


#: chained episodes: (file tag, generator kind, reference class, env id of the drop-in env, constructor keywords, steps)
RESET_CHAINS = [
    ("bup_rs6_a2", "blockedunlockpickup", "BlockedUnlockPickupEnv", "MultiGrid-BlockedUnlockPickup-v0", dict(room_size=6, agents=2, max_steps=7), 72),
    ("bup_rs5_a3", "blockedunlockpickup", "BlockedUnlockPickupEnv", "MultiGrid-BlockedUnlockPickup-v0",
     dict(room_size=5, agents=3, max_steps=5, agent_view_size=5), 60),
    ("bup_rs8_a2", "blockedunlockpickup", "BlockedUnlockPickupEnv", "MultiGrid-BlockedUnlockPickup-v0", dict(room_size=8, agents=2, max_steps=9), 72),
    ("empty_random_6_a3", "empty_random", "EmptyEnv", "MultiGrid-Empty-Random-6x6-v0",
     dict(size=6, agents=3, max_steps=6, agent_view_size=5, agent_start_pos=None), 72),
    ("empty_random_9_a2", "empty_random", "EmptyEnv", "MultiGrid-Empty-Random-6x6-v0",
     dict(size=9, agents=2, max_steps=8, agent_start_pos=None), 72),
]


def record_reset_chains():
    """Chained episodes (tests/golden/resets_chain_*.npz): ONE reference env object, small max_steps, scripted actions, an unseeded
    reset() after every episode end -- what step(auto_reset=True) with device-side generation must reproduce step for step.  Some
    episodes end EARLY: before a step, agent 0 is edited through its AgentState -- BlockedUnlockPickup: handed the target box (the
    hook pays on the next step); Empty: put in front of the goal, facing it, and walked onto it.  The edit is an event of the
    recording (`edit_step`, `edit_row`: agent 0's packed row after it) that a replay applies too.  The draw from env.np_random that
    a reset makes comes after the ending step's action-order draw, at whatever step the episode ends.  Arrays (product layout):

        lay0, npr0 u64[5]            the two generators before the FIRST unseeded reset (both on a pending 32-bit half)
        actions i8[T,A], edit_step i32[K], edit_row u8[K,8]
        obs u8[T,A,v,v,3], dir u8[T,A], reward f64[T,A], terminated u8[T,A], truncated u8[T]      every step's outputs
        grid u8[T,H,W,3], agents u8[T,A,8], npr u64[T,5]     the state the step left (before the reset, where one follows)
        done u8[T]                   an unseeded reset() follows step t;  reset_of i32[T]: its index r (-1: none)
        grid0 u8[R,H,W,3], agents0 u8[R,A,8], obs0 u8[R,A,v,v,3], target u8[R,3], lay_after / npr_after u64[R,5]   reset r (0: the first)
        spec_json                    EnvSpec fields, "gen" (set_layout_generator's keywords), "env_id" / "make" (the drop-in env)"""
    sys.path.insert(0, REPO)
    from multigrid_amd import layouts
    FWD, DONE = 2, 6
    for n, (tag, kind, cls_name, env_id, kw, T) in enumerate(RESET_CHAINS):
        cls = getattr(ref_envs, cls_name)
        cls._default_seed = 0xC4A10 + n
        env = cls(**kw)
        env.reset(seed=n)
        bup = kind == "blockedunlockpickup"
        A = env.num_agents
        lay, npr = env._RandomMixin__np_random, env.np_random
        lay.bit_generator.state, npr.bit_generator.state = _reset_pre_states("chain_" + tag, 3)
        rec = dict(lay0=_gen_words5(lay), npr0=_gen_words5(npr))
        resets = {k: [] for k in ("grid0", "agents0", "obs0", "target", "lay_after", "npr_after")}

        def reset():
            obs, _ = env.reset()
            assert env._RandomMixin__np_random is lay and env.np_random is npr
            resets["grid0"].append(layouts.grid_to_product(grid_with_contents(env)))
            resets["agents0"].append(layouts.pack_agents(agents_with_contents(env)))
            resets["obs0"].append(np.stack([obs[i]["image"] for i in range(A)]))
            resets["target"].append([int(v) for v in np.asarray(env.obj)] if bup else [0, 0, 0])
            resets["lay_after"].append(_gen_words5(lay)); resets["npr_after"].append(_gen_words5(npr))

        reset()
        r = np.random.default_rng(0xAC7 + n)
        actions = r.choice(7, size=(T, A), p=[0.15, 0.15, 0.4, 0.08, 0.06, 0.08, 0.08]).astype(np.int8)
        keys = ("obs", "dir", "reward", "terminated", "truncated", "grid", "agents", "npr", "done", "reset_of")
        log = {k: [] for k in keys}
        edit_step, edit_row = [], []
        episode = 0
        for t in range(T):
            # every other episode ends early, at its 1st, 2nd, 3rd ... step in turn (never at the truncating one)
            if episode % 2 == 1 and env.step_count == (episode // 2) % (env.max_steps - 1):
                a0 = env.agents[0].state
                if bup:
                    a0.carrying = env.obj
                    actions[t, 0] = DONE
                else:
                    a0.pos, a0.dir = (env.width - 3, env.height - 2), 0
                    actions[t, 0] = FWD
                edit_step.append(t); edit_row.append(layouts.pack_agents(agents_with_contents(env))[0])
            obs, rew, term, trunc, _ = env.step({i: int(actions[t, i]) for i in range(A)})
            log["obs"].append(np.stack([obs[i]["image"] for i in range(A)]))
            log["dir"].append([int(obs[i]["direction"]) for i in range(A)])
            log["reward"].append([float(rew[i]) for i in range(A)])
            log["terminated"].append([bool(term[i]) for i in range(A)])
            log["truncated"].append(bool(trunc[0]))
            log["grid"].append(layouts.grid_to_product(grid_with_contents(env)))
            log["agents"].append(layouts.pack_agents(agents_with_contents(env)))
            log["npr"].append(_gen_words5(npr))
            done = bool(env.is_done())
            log["done"].append(done); log["reset_of"].append(len(resets["grid0"]) if done else -1)
            if done:
                reset()
                episode += 1
        rec["actions"] = actions
        rec["edit_step"], rec["edit_row"] = np.asarray(edit_step, dtype=np.int32), np.asarray(edit_row, dtype=np.uint8).reshape(-1, 8)
        for k in keys:
            a = np.asarray(log[k])
            rec[k] = a.astype(np.float64) if k == "reward" else a if k == "npr" else a.astype(np.int32) if k == "reset_of" else a.astype(np.uint8)
        for k, v in resets.items():
            rec[k] = np.asarray(v) if k.endswith("_after") else np.asarray(v).astype(np.uint8)
        gen = dict(kind=kind, room_size=int(kw.get("room_size", 0)), max_hallway_keys=1, max_keys_per_room=2, start=[1, 1, 0])
        mk = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
        rec["spec_json"] = np.array(json.dumps(dict(spec_of_noreset(env, kind if bup else "empty"), gen=gen, env_id=env_id, make=mk)))
        path = os.path.join(OUT, "resets_chain_" + tag + ".npz")
        np.savez_compressed(path, **rec)
        early = int((rec["done"].astype(bool) & ~rec["truncated"].astype(bool)).sum())
        print(f"{'resets_chain_' + tag:40s} T={T} resets={len(resets['grid0'])} early ends={early} truncations={int(rec['truncated'].sum())} "
              f"{os.path.getsize(path) / 1024:.1f} KiB")


def spec_of_noreset(env, kind):
    return dict(
        env_kind=kind, width=int(env.width), height=int(env.height), num_agents=int(env.num_agents),
        view_size=int(env.agents[0].view_size), see_through_walls=bool(env.agents[0].see_through_walls),
        allow_agent_overlap=bool(env.allow_agent_overlap), joint_reward=bool(env.joint_reward),
        success_termination_mode=str(env.success_termination_mode),
        failure_termination_mode=str(env.failure_termination_mode), max_steps=int(env.max_steps))


if __name__ == "__main__":
    if sys.argv[1:] == ["lh_12rooms"]:
        record_lh_12rooms()
    elif sys.argv[1:] == ["conflicts"]:
        record_conflicts()
    else:
        main()
