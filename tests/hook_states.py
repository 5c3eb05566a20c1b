"""Hook-dense states for the env kinds whose step hook does more than BlockedUnlockPickup's (mgx_rules.h: post_step_hook):
RedBlueDoors, LockedHallway (explicit and geometric aux) and the declared `rules` kind.  Plain Python / NumPy over
multigrid_amd.layouts; nothing is read from the reference.  (Test infrastructure.)

`case(name)` -> Case: a spec, a batch of BASE envs, an action script i8[T,BASE,A] and -- RedBlueDoors, LockedHallway -- a visiting
order script u8[T,BASE,A].  Env b starts in scenario b % (number of scenarios) of its kind (the scenarios are listed at the
builders); the first step's actions are mostly the scenario's own, the later ones toggle-heavy random ones.  `step_count` starts
shortly before `max_steps` in a part of the envs, so that they truncate inside the run.

`trajectory(case, ordered)` steps the batch on the CPU oracle once and keeps every step's outputs and post-state; the CPU tests
count the hook events in it (tests/test_hook_states.py: the inputs are not hollow), the GPU tests compare the kernels with it."""
from __future__ import annotations

import dataclasses

import numpy as np

from multigrid_amd import EnvSpec, layouts

BASE = 512
T_STEPS = 10
TOGGLE, FORWARD, PICKUP, LEFT, RIGHT, DROP, DONE = 5, 2, 3, 0, 1, 4, 6
DOOR, KEY, BALL, BOX, GOAL, LAVA = 4, 5, 6, 7, 8, 9
OPEN, CLOSED, LOCKED = 0, 1, 2
RED, GREEN, BLUE, PURPLE = 0, 1, 2, 3
EMPTY = (1, 0, 0)


@dataclasses.dataclass
class Case:
    name: str
    spec: EnvSpec
    state: dict                       # grid u8[B,H,W,3], agents u8[B,A,8], rng u64[B,4], step_count i32[B], aux u8[B,16]
    actions: np.ndarray               # i8[T,B,A]
    hook_order: np.ndarray | None     # u8[T,B,A]
    scenario: np.ndarray              # i32[B]: the scenario every env starts in
    order_can_matter: bool            # False where the hook's result is provably symmetric in the visiting order (see CASES)


def _finish(name, spec, grid, agents, aux, scenario, first, r, with_order, order_can_matter, weights):
    """Common tail: generator words, step counts (a quarter of the envs truncates inside the run), the action and order scripts.
    `first` i8[B,A]: the scenario's own actions of step 0 (-2 = none), played with probability 0.9."""
    B, A = agents.shape[:2]
    rng = r.integers(0, 2 ** 63, size=(B, 4), dtype=np.int64).astype(np.uint64)
    rng[:, 2] |= np.uint64(1)
    sc = np.zeros(B, np.int32)
    late = r.random(B) < 0.25
    sc[late] = spec.max_steps - r.integers(2, T_STEPS, size=int(late.sum()))
    acts = r.choice(np.array(weights, np.int8), size=(T_STEPS, B, A)).astype(np.int8)
    use = (first > -2) & (r.random((B, A)) < 0.9)
    acts[0] = np.where(use, first, acts[0])
    order = None
    if with_order:
        order = np.argsort(r.random((T_STEPS, B, A)), axis=-1).astype(np.uint8)
    st = dict(grid=np.ascontiguousarray(grid), agents=np.ascontiguousarray(agents), rng=rng, step_count=sc, aux=np.ascontiguousarray(aux))
    layouts.check_walled(st["grid"])
    return Case(name, spec, st, acts, order, scenario.astype(np.int32), order_can_matter)


def _agents(B, A):
    ag = np.zeros((B, A, 8), np.uint8)
    ag[..., 0] = np.arange(A) % 6
    ag[..., 5] = 1                                       # empty hands: (empty, 0, 0)
    return ag


# ---------------------------------------------------------------------------------------------------------------- RedBlueDoors
# The 6x6 size: a 12 x 6 grid, the middle room spans x = 3..8, the red door in its left wall (x = 3), the blue one in its right
# wall (x = 8).  Scenarios:
#   0  both doors closed, the agents spread over both doors
#   1  red already open, the agents at the closed blue door: opening it succeeds
#   2  both closed, the agents at the blue door: opening it first fails and sets the stale flag aux[4]
#   3  stale flag set (the grid says open, the door object is closed), a live agent about to toggle it again (ev.unstale); under
#      failure mode "all" agent 0 is the one that failed, so it starts terminated
#   4  every agent stacked at the blue door and toggling: the door ends open when their number is odd, so with two agents it
#      starts open -- the first toggler in the visiting order fails and closes the object, the others find it closed
RBD_SCENARIOS = 5


def redbluedoors(name, A, mode, view, seed):
    spec = EnvSpec(12, 6, A, view, max_steps=24, joint_reward=(A == 3), success_termination_mode="any",
                   failure_termination_mode=mode, env_kind="redbluedoors")
    r = np.random.default_rng(seed)
    B = BASE
    blank = layouts.redbluedoors_blank(6)
    grid = np.repeat(blank[None], B, axis=0)
    ag = _agents(B, A)
    aux = np.zeros((B, 16), np.uint8)
    first = np.full((B, A), -2, np.int8)
    scen = np.arange(B) % RBD_SCENARIOS
    for b in range(B):
        s = scen[b]
        ry, by = int(r.integers(1, 5)), int(r.integers(1, 5))
        red, blue = CLOSED, CLOSED
        at_blue = np.ones(A, bool)
        if s == 0:
            at_blue = r.random(A) < 0.5
        elif s == 1:
            red = OPEN
        elif s == 3:
            blue, aux[b, 4] = OPEN, 1
            red = OPEN if r.random() < 0.3 else CLOSED
            if mode == "all":
                ag[b, 0, 4] = 1
        elif s == 4:
            blue = OPEN if A % 2 == 0 else CLOSED
            red = OPEN if r.random() < 0.25 else CLOSED
        grid[b, ry, 3] = (DOOR, RED, red)
        grid[b, by, 8] = (DOOR, BLUE, blue)
        aux[b, :4] = (8, by, 3, ry)
        for a in range(A):
            ag[b, a, 1:4] = (0, 7, by) if at_blue[a] else (2, 4, ry)
            first[b, a] = TOGGLE
    return _finish(name, spec, grid, ag, aux, scen, first, r, True, mode == "all", [5, 5, 5, 5, 0, 1, 2, 6, -1])


# --------------------------------------------------------------------------------------------------------------- LockedHallway
# Three columns of rooms of `rs` cells; the hallway is the middle column, door k = (row k // 2, side k % 2) sits mid-wall at
# x = rs - 1 (left) or 2 (rs - 1) (right).  Every agent holds the key of the door it faces unless said otherwise.  Scenarios:
#   0  a first unlock: agent 0 with the key at a locked door, the others at doors of their own (in every other env of the scenario
#      agent 1 stands with agent 0, without a key)
#   1  a door that is already unlocked (closed or open, its mask bit set) and toggled again: no reward
#   2  two agents at one locked door, both toggling (one key): the first in the visiting order is paid (own rewards)
#   3  agent 0 unlocks while the last agent walks onto a goal (even envs) or lava (odd) in the same step: `+=` on the base reward
#   4  one unlock short of the forced termination aux[15]: the mask holds target - 1 doors, agent 0 at a locked one with its key
#   5  every agent at a door of its own with its key
LH_SCENARIOS = 6


def lockedhallway(name, rooms, rs, A, joint, view, seed):
    rows_n = rooms // 2
    W, H = 3 * (rs - 1) + 1, rows_n * (rs - 1) + 1
    spec = EnvSpec(W, H, A, view, max_steps=24, joint_reward=joint, env_kind="lockedhallway")
    r = np.random.default_rng(seed)
    B = BASE
    grid = np.zeros((B, H, W, 3), np.uint8)
    ag = _agents(B, A)
    aux = np.zeros((B, 16), np.uint8)
    first = np.full((B, A), -2, np.int8)
    scen = np.arange(B) % LH_SCENARIOS

    def door_xy(k):
        return (rs - 1) * (1 + k % 2), (k // 2) * (rs - 1) + (rs - 1) // 2

    protos = [layouts.lockedhallway_layout(rooms, rs, 1, 2, 1, np.random.default_rng(seed * 100 + k), np.random.default_rng(k))[0]
              for k in range(8)]
    for b in range(B):
        s = scen[b]
        g = protos[int(r.integers(len(protos)))].copy()
        hall = slice(rs, 2 * (rs - 1))
        sub = g[1:H - 1, hall]
        sub[sub[..., 0] == KEY] = EMPTY                                          # keys off the hallway: the agents stand there
        a0 = layouts.make_aux("lockedhallway", g)
        geo = bool(a0[0] & 0x80)
        target = int(a0[4]) if geo else rooms
        mask = 0

        def unlock(k):
            nonlocal mask
            x, y = door_xy(k)
            g[y, x, 2] = OPEN if r.random() < 0.5 else CLOSED
            mask |= 1 << k

        def stand(a, k, key=True):
            x, y = door_xy(k)
            ag[b, a, 1:4] = (2, x + 1, y) if k % 2 == 0 else (0, x - 1, y)
            ag[b, a, 5:8] = (KEY, g[y, x, 1], 0) if key else EMPTY
            first[b, a] = TOGGLE

        doors = r.permutation(rooms)
        if s == 4:
            for k in doors[1:target]:
                unlock(int(k))
        elif s == 1:
            unlock(int(doors[0]))
        for a in range(A):
            stand(a, int(doors[a % rooms]))
        if s == 2 or (s == 0 and (b // LH_SCENARIOS) % 2):
            stand(1, int(doors[0]), key=False)
            if A > 2 and r.random() < 0.5:
                stand(2, int(doors[0]), key=False)
        if s == 3:
            k = int(doors[0])
            x, y = door_xy(k)
            gy = y + 1 if y + 1 < H - 1 and g[y + 1, rs, 0] == 1 and g[y + 1, rs + 1, 0] == 1 else y - 1
            g[gy, rs + 1] = (GOAL, GREEN, 0) if b % 2 == 0 else (LAVA, 0, 0)
            ag[b, A - 1, 1:4] = (0, rs, gy)
            ag[b, A - 1, 5:8] = EMPTY
            first[b, A - 1] = FORWARD
        grid[b] = g
        aux[b] = a0
        aux[b, 1] = mask & 0xff
        if geo:
            aux[b, 2] = mask >> 8
    return _finish(name, spec, grid, ag, aux, scen, first, r, True, not joint, [5, 5, 5, 5, 0, 1, 2, 6, -1])


# ----------------------------------------------------------------------------------------------------------------------- rules
# The declared hook (include/mgx.h: MGX_KIND_RULES), with the rule sets of the user-defined envs of tests/custom_envs.py:
#   fetchtrap   {carries (ball, purple) -> success; toggles_at (the red trap door) while open -> failure}: a wall across the grid at
#               y = H - 3 with the trap door in it; agents beside the purple ball (pickup: carries succeeds), beside the green decoy
#               (carries fails), above the closed trap (toggling opens it: failure), above the open trap (toggling shuts it: the
#               condition fails) and toggling somewhere else
#   twinballs   {carries (ball, purple) -> success}, success mode "all", joint rewards: purple balls and green ones
#   bup         BlockedUnlockPickup as the one rule {carries (box, colour) -> success} on its own generated layouts: agents beside
#               the target box, and beside the ball that blocks the door
RULE_SCENARIOS = 5


def rules(name, which, A, view, seed):
    r = np.random.default_rng(seed)
    B = BASE
    scen = np.arange(B) % RULE_SCENARIOS
    first = np.full((B, A), -2, np.int8)
    ag = _agents(B, A)
    aux = np.zeros((B, 16), np.uint8)
    if which == "bup":
        spec = EnvSpec(11, 6, A, view, max_steps=24, joint_reward=True, env_kind="rules")
        grid = np.zeros((B, 6, 11, 3), np.uint8)
        for b in range(B):
            rr = np.random.default_rng(seed * 1000 + b % 40)
            g, a, tgt = layouts.blockedunlockpickup_layout(6, A, rr, rr)
            ag[b] = a
            aux[b] = layouts.rules_aux([("carries", int(tgt[0]), int(tgt[1]), "success")])
            for i in range(A):
                want = BOX if (scen[b] + i) % 2 == 0 else BALL
                (y, x), = np.argwhere(g[..., 0] == want)[:1]
                for d, (dx, dy) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):
                    if g[y - dy, x - dx, 0] == 1:
                        ag[b, i, 1:4] = (d, x - dx, y - dy)
                        first[b, i] = PICKUP
                        break
            grid[b] = g
        return _finish(name, spec, grid, ag, aux, scen, first, r, False, False, [3, 3, 4, 0, 1, 2, 5, 6, -1])
    S = 9
    grid = np.zeros((B, S, S, 3), np.uint8)
    grid[..., 0] = 1
    grid[:, 0], grid[:, -1], grid[:, :, 0], grid[:, :, -1] = (2, 5, 0), (2, 5, 0), (2, 5, 0), (2, 5, 0)
    if which == "twinballs":
        spec = EnvSpec(S, S, A, view, max_steps=24, joint_reward=True, success_termination_mode="all", env_kind="rules")
        for b in range(B):
            aux[b] = layouts.rules_aux([("carries", BALL, PURPLE, "success")])
            for i in range(A):
                x = 1 + 2 * i
                grid[b, 2, x] = (BALL, PURPLE if (scen[b] + i) % 3 else GREEN, 0)
                ag[b, i, 1:4] = (1, x, 1)
                first[b, i] = PICKUP
            grid[b, int(r.integers(4, S - 1)), int(r.integers(1, S - 1))] = (BALL, PURPLE, 0)
        return _finish(name, spec, grid, ag, aux, scen, first, r, False, False, [3, 3, 4, 4, 0, 1, 2, 6, -1])
    spec = EnvSpec(S, S, A, view, max_steps=24, failure_termination_mode="all", env_kind="rules")
    for b in range(B):
        s = scen[b]
        tx = int(r.integers(1, S - 1))
        grid[b, S - 3, :] = (2, 5, 0)
        grid[b, S - 3, tx] = (DOOR, RED, OPEN if s == 3 else CLOSED)
        aux[b] = layouts.rules_aux([("carries", BALL, PURPLE, "success"), ("toggles_at", tx, S - 3, "failure", "open")])
        px, gx = (int(v) for v in r.permutation(np.arange(1, S - 1))[:2])
        grid[b, 2, px] = (BALL, PURPLE, 0)
        grid[b, 2, gx] = (BALL, GREEN, 0)
        for i in range(A):
            k = (s + i) % RULE_SCENARIOS
            if k == 0:
                ag[b, i, 1:4] = (1, px, 1); first[b, i] = PICKUP
            elif k == 1:
                ag[b, i, 1:4] = (1, gx, 1); first[b, i] = PICKUP
            elif k in (2, 3):
                ag[b, i, 1:4] = (1, tx, S - 4); first[b, i] = TOGGLE
            else:
                ag[b, i, 1:4] = (int(r.integers(4)), int(r.integers(1, S - 1)), 3); first[b, i] = TOGGLE
    return _finish(name, spec, grid, ag, aux, scen, first, r, False, False, [5, 5, 3, 4, 0, 1, 2, 6, -1])


# name -> builder.  Views 3, 7 and 9; 2 - 4 agents.  The visiting order can change a result only where the hook treats the first
# toggler differently: RedBlueDoors under failure mode "all" (under "any" whoever fails first ends every agent's episode, and the
# stale flag is set either way), LockedHallway with own rewards (a joint reward pays every agent whoever unlocks).
CASES = {
    "rbd_a2_all_v7": lambda: redbluedoors("rbd_a2_all_v7", 2, "all", 7, 11),
    "rbd_a3_all_v3": lambda: redbluedoors("rbd_a3_all_v3", 3, "all", 3, 12),
    "rbd_a2_any_v9": lambda: redbluedoors("rbd_a2_any_v9", 2, "any", 9, 13),
    "rbd_a3_any_v7": lambda: redbluedoors("rbd_a3_any_v7", 3, "any", 7, 14),
    "lh2_a2_own_v7": lambda: lockedhallway("lh2_a2_own_v7", 2, 5, 2, False, 7, 21),
    "lh2_a3_joint_v3": lambda: lockedhallway("lh2_a3_joint_v3", 2, 5, 3, True, 3, 22),
    "lh8_a3_own_v9": lambda: lockedhallway("lh8_a3_own_v9", 8, 4, 3, False, 9, 23),
    "lh8_a4_joint_v7": lambda: lockedhallway("lh8_a4_joint_v7", 8, 4, 4, True, 7, 24),
    "lh12_a3_own_v7": lambda: lockedhallway("lh12_a3_own_v7", 12, 4, 3, False, 7, 25),
    "lh12_a2_joint_v9": lambda: lockedhallway("lh12_a2_joint_v9", 12, 4, 2, True, 9, 26),
    "rules_fetchtrap_a2_v7": lambda: rules("rules_fetchtrap_a2_v7", "fetchtrap", 2, 7, 31),
    "rules_twinballs_a3_v9": lambda: rules("rules_twinballs_a3_v9", "twinballs", 3, 9, 32),
    "rules_bup_a2_v3": lambda: rules("rules_bup_a2_v3", "bup", 2, 3, 33),
}
NAMES = list(CASES)
_CASES, _TRAJ = {}, {}


def case(name) -> Case:
    if name not in _CASES:
        _CASES[name] = CASES[name]()
    return _CASES[name]


def kind_of(name) -> str:
    return {"rbd": "redbluedoors", "lh2": "lockedhallway", "lh8": "lockedhallway", "lh12": "lockedhallway", "rules": "rules"}[name.split("_")[0]]


def trajectory(name, ordered: bool = True) -> list:
    """The oracle's run of the case: a list over the steps of dict(obs, dir, reward, terminated, truncated -- the outputs -- and
    grid, agents, rng, step_count, aux -- the state after the step).  ordered=False: ascending visiting order.  Computed once."""
    from oracle import binding as ob
    c = case(name)
    ordered = ordered and c.hook_order is not None
    key = (name, ordered)
    if key not in _TRAJ:
        st = {k: v.copy() for k, v in c.state.items()}
        sd = c.spec.as_dict()
        out = []
        for t in range(c.actions.shape[0]):
            o = ob.step_batch(sd, st["grid"], st["agents"], st["rng"], st["step_count"], np.ascontiguousarray(c.actions[t]), st["aux"],
                              nthreads=4, hook_order=np.ascontiguousarray(c.hook_order[t]) if ordered else None)
            rec = dict(zip(("obs", "dir", "reward", "terminated", "truncated"), (x.copy() for x in o)))
            rec.update({k: v.copy() for k, v in st.items()})
            out.append(rec)
        _TRAJ[key] = out
    return _TRAJ[key]
