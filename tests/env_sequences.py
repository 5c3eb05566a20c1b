"""Random call sequences through BatchedMultiGridEnv: the driver of tests/test_env_sequences.py (two oracle-backed envs, no GPU) and
tests/test_env_sequences_gpu.py (HIP against the oracle).  No tests in here.

  * `make_ops(form, B, n_ops, seed)` lists every call up front, arguments included (NumPy values).  Whether a call is legal is decided
    from host-known facts alone -- the form, whether the accounting is on, B >= 128, which snapshots and graphs are kept and what
    they carry -- never from a result: two envs given one list do the same thing, and (form, B, n_ops, seed) names a failure.
  * `apply(env, op, ctx)` performs one call on either kind of env (the GPU-only kinds have an eager equivalent on the oracle).
  * `compare(a, b, ...)` holds two envs to each other byte for byte; `invariants(env)` are the layout marker's two rules;
    `SeqOracle` is the CPU model of every launcher -- CopyOracle(StatsOracle(SelectOracle(OracleBackend))) -- with a one-hot gen_obs,
    an accounting of its own fed from what the launches hand back (`shadow`: what EpisodeStats must hold whatever the host logic
    called), and the census of what a run went through.
  * the query layer (`make_ops(..., queries=True)`): after every call of the list zero to two READ-ONLY calls -- state_key, obs_key,
    action_mask, distance_field / agent_distance, the same on a kept snapshot, a key table fed from state keys, a selection over the
    batch, and (GPU) all of them captured into one graph -- whose arguments come from a generator of their own: the list without
    them is the list there was before (`without_queries`).  Their launchers on the oracle are the models of the queries' own test
    files (KeyOracle, MaskOracle, DistOracle, KeyTableModel, SelectModel); what is under test is the host logic in front of the
    launch: `_copy_entry`, `_row_set`, the snapshot's `_row_set`, `join()`.
  * the hook forms (HOOK_FORMS): RedBlueDoors, LockedHallway, Playground's generator and the declared rules, whose steps rewrite
    `aux` -- the 16 hook-state bytes that EnvSnapshot, fork, state_dict, the candidate slots and a pool's `auxs` must carry.  Random
    walks do not reach hook events, so the starts do: the pool forms restart from hook-dense states of tests/hook_states.py with
    their aux (`hook_pool`).  The stepping calls of the RedBlueDoors and LockedHallway forms carry a `hook_order`, which sends
    step() through its slow entry.  The census (`SeqOracle._hook_census`, HOOK_NEED) asks for what these forms are there to meet."""
import weakref

import numpy as np
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib, layouts
from multigrid_amd.key_table import KeyInsert
from multigrid_amd.select import Selection
from oracle import binding as ob
from tests import hook_states as hs
from tests import util
from tests.test_distance import DistOracle
from tests.test_env_snapshot import TRIO
from tests.test_episode_stats import model_restart, model_stats, new_state
from tests.test_key_table import KeyTableModel
from tests.test_select import SelectModel, threshold
from tests.test_state_key import SALTS, KeyOracle

NONE, BEFORE, AFTER = _lib.RESTART_NONE, _lib.RESTART_BEFORE, _lib.RESTART_AFTER
STATE = ("_cells", "agents", "rng", "step_count")
OUTPUTS = ("obs", "dir", "reward", "terminated", "truncated")
#: the forms of the hook kinds whose step rewrites `aux`, the 16 hook-state bytes (RedBlueDoors, LockedHallway, the declared rules), and
#: Playground's generator: the generator forms start their episodes on the device (one candidate per env; Playground falls back to
#: "between"), the pool forms from hook-dense states of tests/hook_states.py -- one or two actions before a success, a failure or an
#: outcome that depends on the visiting order, as `pool1`'s start is one cell before the goal
HOOK_FORMS = ("rbd_candidates", "rbd_pool", "lh_candidates", "lh_pool", "playground_between", "rules_pool", "lh12_pool")
FORMS = ("plain", "pool1", "pool4_objects", "pool_compact", "gen", "gen_candidates", "gen_between", "bup_candidates") + HOOK_FORMS
#: the batch whose launches READ the layout marker (more than 2048 wavefronts, one layout): tests/test_env_sequences_gpu.py
BIG_FORMS = ("big_empty1", "big_objects1")
#: `plain` and `pool1` on shapes of their own -- grids that are not square --, which the HIP env steps on a kernel compiled at run time
#: (make_env(specialise=True); a registration serves every env of its geometry for the rest of the process: no other form, and no
#: other test file, uses these shapes): tests/test_jit_forms_gpu.py
JIT_FORMS = ("plain_jit", "pool1_jit")
#: a form's place in this list seeds its lists: new forms go to the END (the lists of the others must not change by one argument)
SEED_ORDER = FORMS[:8] + BIG_FORMS + JIT_FORMS + HOOK_FORMS
PLAIN_FORMS = ("plain", "plain_jit")                         # no restart source: load_state alone
POOL1_FORMS = ("pool1", "pool1_jit")
#: the hook pool forms and the case of tests/hook_states.py whose 512 base states their pools are taken from
#: (lh_pool: two rooms, the explicit aux -- door positions listed; lh12_pool: twelve rooms and three agents, the geometric aux, whose
#: unlocked-door mask has a second byte)
HOOK_CASE = {"rbd_pool": "rbd_a2_all_v7", "lh_pool": "lh2_a2_own_v7", "rules_pool": "rules_fetchtrap_a2_v7", "lh12_pool": "lh12_a3_own_v7"}
HOOK_POOL_FORMS = tuple(HOOK_CASE)
POOL_FORMS = ("pool1", "pool4_objects", "pool_compact") + BIG_FORMS + ("pool1_jit",) + HOOK_POOL_FORMS
GEN_FORMS = ("gen", "gen_candidates", "gen_between", "bup_candidates", "rbd_candidates", "lh_candidates", "playground_between")
STAGED_FORMS = ("gen_candidates", "gen_between", "bup_candidates", "rbd_candidates", "lh_candidates", "playground_between")
#: the forms whose step hook visits the agents in the order of the caller's actions dict: their stepping calls carry a `hook_order`;
#: of these the pool forms are the ORDERED ones -- RedBlueDoors under failure mode "all", LockedHallway with own rewards, where the
#: first toggler is treated differently (hook_states.CASES)
ORDER_FORMS = ("rbd_candidates", "rbd_pool", "lh_candidates", "lh_pool", "lh12_pool")
ORDERED_POOL_FORMS = ("rbd_pool", "lh_pool", "lh12_pool")
RBD_FORMS = ("rbd_candidates", "rbd_pool")
#: the env kinds whose step hook rewrites `aux` or reads a table in it (BlockedUnlockPickup's reads three constant bytes)
HOOK_KINDS = ("redbluedoors", "lockedhallway", "rules")
SPECS = {
    "plain": EnvSpec(8, 8, 3, 5, max_steps=12),
    "pool1": EnvSpec(5, 5, 2, 3, max_steps=6),
    "pool4_objects": EnvSpec(16, 16, 4, 7, max_steps=8),
    "pool_compact": EnvSpec(5, 5, 2, 3, max_steps=6, cell_bytes=1),
    "gen": EnvSpec(5, 5, 2, 3, max_steps=6),
    "gen_candidates": EnvSpec(5, 5, 2, 3, max_steps=6),
    "gen_between": EnvSpec(5, 5, 2, 3, max_steps=6),
    "bup_candidates": EnvSpec(11, 6, 2, 7, max_steps=8, joint_reward=True, env_kind="blockedunlockpickup"),
    "big_empty1": EnvSpec(16, 16, 4, 7, max_steps=8),
    "big_objects1": EnvSpec(16, 16, 4, 7, max_steps=8),
    "plain_jit": EnvSpec(7, 6, 3, 5, max_steps=12),
    "pool1_jit": EnvSpec(6, 5, 2, 3, max_steps=6),
    "rbd_candidates": EnvSpec(8, 4, 2, 3, max_steps=8, env_kind="redbluedoors"),
    "rbd_pool": EnvSpec(12, 6, 2, 7, max_steps=24, failure_termination_mode="all", env_kind="redbluedoors"),
    "lh_candidates": EnvSpec(13, 9, 2, 3, max_steps=8, joint_reward=True, env_kind="lockedhallway"),
    "lh_pool": EnvSpec(13, 5, 2, 7, max_steps=24, env_kind="lockedhallway"),
    "playground_between": EnvSpec(13, 7, 2, 3, max_steps=8),
    "rules_pool": EnvSpec(9, 9, 2, 7, max_steps=24, failure_termination_mode="all", env_kind="rules"),
    "lh12_pool": EnvSpec(10, 19, 3, 7, max_steps=24, env_kind="lockedhallway"),
}
FIRST_ENV = {"pool4_objects": 11, "gen_between": 11, "bup_candidates": 11, "rbd_pool": 11, "lh_candidates": 11}
#: the pool sizes a form alternates between when `pool_replace` gives it another K
POOL_K = {"pool1": (1, 2), "pool4_objects": (4, 3), "pool_compact": (2, 3), "big_empty1": (1, 2), "big_objects1": (1, 2),
          "pool1_jit": (1, 2),
          # (the hook pools: eleven starts -- ten consecutive base states, every scenario of the kind among them, and the twin of one
          # that differs from it in `aux` alone --, or ONE: the pool size at which set_layout_pool() and reset() arm the marker of an
          # oracle-backed env, too)
          "rbd_pool": (11, 1), "lh_pool": (11, 1), "rules_pool": (11, 1), "lh12_pool": (13, 1)}
#: the commonest object type of a form's grids, what `q_select` scores by: the goal of the Empty layouts, a door where the grids are
#: util.random_state's (three of its ten kinds of cell) and in BlockedUnlockPickup
COMMON_TYPE = {f: (4 if f in ("plain", "plain_jit", "pool4_objects", "big_objects1", "bup_candidates") else 8) for f in SPECS}
COMMON_TYPE.update({f: 4 for f in HOOK_FORMS}, rules_pool=6)           # (doors; the balls of the fetch-and-trap rules)
#: (type, color, state) triples a cell edit writes: every cell format holds them, and an agent may stand on each (the edit may land
#: under one): empty, floors, lava, a goal
EDIT_CELLS = np.array([[1, 0, 0], [3, 3, 0], [3, 1, 0], [9, 0, 0], [8, 1, 0], [3, 4, 0]], np.uint8)
#: what a refilled small pool puts on its layouts: a ball, a key, a box
POOL_OBJECTS = np.array([[6, 2, 0], [5, 1, 0], [7, 4, 0]], np.uint8)
MAX_SNAPS = 4
#: kinds that only the HIP backend has a form of its own for; the oracle runs their eager equivalent
GPU_KINDS = ("capture_replay", "graph_again", "persistent", "step_chains")
#: what a recorded stretch may hold: functions of the env state and the call's arguments (the time machine); `one_hot_obs` is a
#: function of the `obs` buffer, which is no part of a snapshot
PURE_KINDS = ("step", "step_one_hot", "rollout", "reset_done", "reset", "snapshot", "snapshot_out", "restore", "fork", "edit", "seed",
              "gen_obs", "full_obs", "capture_replay", "step_chains", "q_state_key", "q_action_mask", "q_distance", "q_snap", "q_select")
#: the query layer: calls that write nothing.  ROW_QUERIES go through `_row_set` of the env (q_table and q_select begin with one), so
#: each of them may be the first consumer of pending sub-shard chains; `q_obs_key` reads the `obs` buffer and `q_table` a table of
#: its own: not pure
ROW_QUERIES = ("q_state_key", "q_action_mask", "q_distance")
QUERY_KINDS = ROW_QUERIES + ("q_obs_key", "q_snap", "q_table", "q_select", "q_graph", "q_graph_again")
FIRST_CONSUMERS = ROW_QUERIES + ("q_table", "q_select")
GPU_QUERY_KINDS = ("q_graph", "q_graph_again")
QUERY_WEIGHTS = {"q_state_key": 3, "q_obs_key": 1.5, "q_action_mask": 3, "q_distance": 4, "q_snap": 3.5, "q_table": 4, "q_select": 1.5,
                 "q_graph": 1, "q_graph_again": 1.5}
#: how many queries follow a call
QUERY_COUNT_P = (0.3, 0.4, 0.3)
#: rows per query.  The oracle's query models walk their rows in Python: at 40 rows, a whole batch every eighth query and a
#: selection as often as a row query the GPU cases took 2.5 to 3 times their time without the layer (profiles/env_sequences_queries.txt);
#: the rows were cut, not the queries
MAX_QUERY_ROWS = 24
#: the object types a distance query may name (goal, key, ball, box, door, lava), and per form the commonest one: what `q_select` scores by
SOURCE_TYPES = (8, 5, 6, 7, 4, 9)
THROUGH = ("closed", "locked", "objects")
TABLE_CAPACITY = 1 << 12
#: `q_select` at the batch that reads the marker: one pass over the first envs only
SELECT_MAX = 4096
MAX_QUERY_GRAPHS = 3
#: relative frequencies; every legal kind must run at least three times over a form's seeds (the census of the tests)
WEIGHTS = {"step": 8, "step_one_hot": 2, "rollout": 3, "reset_done": 2, "reset": 3, "snapshot": 4, "snapshot_out": 2, "restore": 5,
           "fork": 2, "edit": 3, "load_state_dict": 1.6, "pool_refill": 1.6, "pool_replace": 1.4, "track": 3.0, "reset_totals": 2.6,
           "stats_lsd": 2.6, "seed": 2, "gen_obs": 2, "full_obs": 2, "one_hot_obs": 2, "split": 2, "capture_replay": 2.5,
           "graph_again": 4, "persistent": 3, "step_chains": 4}


# ---- the oracle launcher ------------------------------------------------------------------------------------------------------------

class SeqOracle(KeyOracle, DistOracle, KeyTableModel, SelectModel):
    """The CPU model of every launcher -- the queries' launchers are the models of their own test files, composed: KeyOracle and
    DistOracle (which is MaskOracle too) over the one CopyOracle, the key table's and the selection's mixins --, and what watches a run:

    shadow   the accounting's tensors as they must be, or None while it is off: updated HERE from what each stepping / restart launch
             hands back, by the sequential model -- not by the accounting calls the host logic makes, which it checks.  A restore
             takes the running trio of the rows it wrote from the env (the env copy is held to its own model elsewhere).
    census   what happened: restarts by truncation / termination, a restored env that crossed an episode end, ...; for the hook kinds
             (HOOK_KINDS) what the step hooks met -- `_hook_census` --, whether a restore, a fork or a generated restart wrote
             another `aux` than the env had, and where a visiting order decided an outcome
    Sub-shards of split() share the launcher: their rows are found by the storage offset of their `step_count` view."""

    def __init__(self, spec):
        super().__init__(spec)
        self.shadow, self.census, self.env = None, {}, None
        self._nested, self._faking = 0, False
        self.restored, self.forking = None, False        # (forking: apply() is inside env.fork(), whose copy is a restore)
        self.ordered_launches = 0                        # (step launches that came with a visiting order)

    def attach(self, env):
        self.env = weakref.ref(env)
        self.restored = np.zeros(env.batch, bool)

    def _count(self, what, n=1):
        if n:
            self.census[what] = self.census.get(what, 0) + int(n)

    def _rows(self, step_count, B):
        lo = int(step_count.storage_offset())
        return slice(lo, lo + B)

    def _shadow_rows(self, rows):
        return {k: v[rows] for k, v in self.shadow.items()}

    def gen_obs(self, B, grid, agents, obs, dirs, one_hot: bool = False):
        if not one_hot:
            return super().gen_obs(B, grid, agents, obs, dirs)
        o, d = ob.gen_obs_batch(self.d, self._g3(grid), agents.numpy(), self.nthreads)
        obs.copy_(torch.from_numpy(ob.one_hot(o)))
        dirs.copy_(torch.from_numpy(d))

    def step(self, B, grid, agents, rng, step_count, actions, target, err, obs, dirs, reward, terminated, truncated, **kw):
        ar = kw.get("auto_reset")
        self.ordered_launches += int(kw.get("hook_order") is not None)
        self._nested += 1
        try:
            if self.spec.env_kind in HOOK_KINDS:
                # (the fused form IS reset_done, then the step -- util.OracleBackend.step: taken apart here, so that the state the
                # hook meets is at hand)
                if ar is not None:
                    self.reset_done(B, ar[0], ar[1], grid, agents, step_count, target, ar[2], ar[3])
                kw = {k: v for k, v in kw.items() if k != "auto_reset"}
                pre = {"grid": self._g3(grid).copy(), "agents": agents.numpy().copy(), "rng": rng.numpy().copy(),
                       "step_count": step_count.numpy().copy(), "aux": target.numpy().copy()}
            super().step(B, grid, agents, rng, step_count, actions, target, err, obs, dirs, reward, terminated, truncated, **kw)
            if self.spec.env_kind in HOOK_KINDS:
                self._hook_census(pre, actions.numpy(), kw.get("hook_order"), self._g3(grid), agents.numpy(), target.numpy(),
                                  reward.numpy(), terminated.numpy())
        finally:
            self._nested -= 1
        if self.shadow is not None and self._nested == 0:
            model_stats(self._shadow_rows(self._rows(step_count, B)), reward.numpy(), terminated.numpy(), truncated.numpy(),
                        ar[3].numpy() if ar is not None else None, BEFORE if ar is not None else NONE)

    def _hook_census(self, pre, act, hook_order, grid, agents, aux, reward, terminated):
        """What one step of a hook kind went through, from the state before it (`pre`, behind the restarts of a fused step) and
        after it; the event classes are those of tests/test_hook_states.py.  A step with a visiting order is taken once more on a
        copy, in ascending order: the envs whose state or outputs differ are where the order decided something."""
        B = act.shape[0]
        b = np.arange(B)
        self._count("aux_changed_by_a_step", (pre["aux"] != aux).any(axis=1).sum())
        paid = reward > 0
        if self.spec.env_kind == "redbluedoors":
            self._count("hook_success", (paid & (act == hs.TOGGLE)).any(axis=1).sum())        # (no other toggle is paid)
            self._count("hook_failure", ((pre["aux"][:, 4] == 0) & (aux[:, 4] == 1)).sum())    # (it leaves the stale flag behind)
        if self.spec.env_kind == "rules":
            want = pre["aux"][:, 2].astype(np.int64) | (pre["aux"][:, 3].astype(np.int64) << 8)
            carry = agents[..., 5].astype(np.int64) | (agents[..., 6].astype(np.int64) << 8)
            self._count("rule_carries_fired", ((carry == want[:, None]) & paid).any(axis=1).sum())
            d = agents[..., 1] & 3
            fx = agents[..., 2].astype(np.int64) + np.array([1, 0, -1, 0])[d]
            fy = agents[..., 3].astype(np.int64) + np.array([0, 1, 0, -1])[d]
            at = (act == hs.TOGGLE) & (fx == pre["aux"][:, None, 7]) & (fy == pre["aux"][:, None, 8])
            door_open = (grid[b, pre["aux"][:, 8], pre["aux"][:, 7], 0] == hs.DOOR) & (grid[b, pre["aux"][:, 8], pre["aux"][:, 7], 2] == hs.OPEN)
            newly = (pre["agents"][..., 4] == 0) & (agents[..., 4] != 0) & ~paid
            self._count("rule_toggles_at_fired", (at & door_open[:, None] & newly).any(axis=1).sum())
        if hook_order is None:
            return
        self._count("stepped_with_hook_order_while_tracking_episodes", int(self.shadow is not None))
        c = {k: v.copy() for k, v in pre.items()}
        out = ob.step_batch(self.d, c["grid"], c["agents"], c["rng"].view(np.uint64), c["step_count"], act, c["aux"], self.nthreads,
                            hook_order=None)
        differs = (c["grid"] != grid).any(axis=(1, 2, 3)) | (c["agents"] != agents).any(axis=(1, 2)) | (c["aux"] != aux).any(axis=1) \
            | (out[2].view(np.int64) != reward.view(np.int64)).any(axis=1) | (out[3] != terminated).any(axis=1)
        self._count("hook_order_changed_the_outcome", differs.sum())

    def _restarting(self, B, agents, step_count):
        """(before a done-based restart) who restarts, and why"""
        rows = self._rows(step_count, B)
        term = (agents[:, :, 4] != 0).all(dim=1).numpy()
        trunc = (step_count >= self.spec.max_steps).numpy() & ~term
        if not self._faking:
            self._count("restart_by_truncation", trunc.sum())
            self._count("restart_by_termination", term.sum())
            if self.restored is not None:
                self._count("restored_env_crossed_an_episode_end", (self.restored[rows] & (term | trunc)).sum())
        return rows

    def _restarted(self, rows, step_count, B, was_reset):
        if self.restored is not None:
            self.restored[rows][was_reset.numpy().astype(bool)] = False
        if self.shadow is not None and self._nested == 0:
            model_restart(self._shadow_rows(rows), was_reset.numpy())

    def reset_done(self, B, first_env, pool, grid, agents, step_count, target, episode, was_reset):
        rows = self._restarting(B, agents, step_count)
        super().reset_done(B, first_env, pool, grid, agents, step_count, target, episode, was_reset)
        self._restarted(rows, step_count, B, was_reset)

    def reset_generate(self, B, gen, grid, agents, rng, step_count, aux, episode, was_reset):
        rows = self._restarting(B, agents, step_count)
        super().reset_generate(B, gen, grid, agents, rng, step_count, aux, episode, was_reset)
        if aux is not None and (gen.get("stage") or {}).get("aux") is not None and not self._faking:
            # (an episode end of a staged generator of a hook kind: on the device the adoption of a slot, its aux included)
            self._count("adoption_of_a_slot_with_aux", (was_reset.bool() & (aux != 0).any(dim=1)).sum())
        self._restarted(rows, step_count, B, was_reset)

    def _as_done(self, sel, agents, step_count, call):
        self._faking = True
        try:
            super()._as_done(sel, agents, step_count, call)
        finally:
            self._faking = False

    def env_copy(self, n, src, src_rows, src_idx, dst, dst_rows, dst_idx, stage_tag, stage_mode, marker_fill, bad):
        env = self.env() if self.env is not None else None
        into_env = env is not None and dst["cells"].data_ptr() == env._cells.data_ptr()
        old_aux = dst["aux"].clone() if into_env else None
        super().env_copy(n, src, src_rows, src_idx, dst, dst_rows, dst_idx, stage_tag, stage_mode, marker_fill, bad)
        if not into_env:
            return                                         # (a snapshot: the env is the source)
        self._count("fork_copied_a_different_aux" if self.forking else "restore_wrote_a_different_aux",
                    (old_aux != dst["aux"]).any(dim=1).sum())
        ids = np.arange(n) if dst_idx is None else dst_idx.numpy()
        self.restored[ids[(ids >= 0) & (ids < dst_rows)]] = True
        if dst.get("cur_length") is not None and src.get("cur_length") is None:
            self._count("restored_row_without_the_running_episode", n)
        if self.shadow is not None:
            for m in TRIO:
                self.shadow[m][...] = env._stats.tensors[m].numpy()


# ---- the forms ----------------------------------------------------------------------------------------------------------------------

def object_pool(spec, K, seed):
    st = util.random_state(spec, K, seed, density=0.3, terminated_p=0.0)
    return st["grid"], st["agents"], None


def empty_start(spec, pos=(1, 1), direction=0):
    """layouts.empty_layout for a grid that may be wider than high: the square layout's upper rows, closed by a wall, the goal in
    the new far corner"""
    W, H = spec.width, spec.height
    g, a = layouts.empty_layout(W, spec.num_agents, agent_start_pos=pos, agent_start_dir=direction)
    if H != W:
        assert H < W and pos[1] < H - 1
        wall, goal, empty = g[0, 0].copy(), g[W - 2, W - 2].copy(), g[1, 1].copy()
        g[W - 2, W - 2] = empty
        g = g[:H].copy()
        g[H - 1] = wall
        g[H - 2, W - 2] = goal
    return g, a


def start_pool(spec):
    """test_episode_stats.empty_pool for any such grid: the reference's start, and one cell before the goal, facing it"""
    g0, a0 = empty_start(spec)
    g1, a1 = empty_start(spec, (spec.width - 3, spec.height - 2), 0)
    return np.stack([g0, g1]), np.stack([a0, a1])


def small_pool(spec, K, r):
    """K starts of a small Empty grid with one more object on it: the layouts differ in their CELLS (the two of
    test_episode_stats.empty_pool differ in the agents only); some starts face the goal"""
    gs, ags = [], []
    for _ in range(K):
        pos = [(1, 1), (2, 3), (3, 2), (2, 2)][int(r.integers(0, 4))]
        g, a = empty_start(spec, pos, int(r.integers(0, 4)))
        while True:
            x, y = (int(v) for v in r.integers(1, spec.width - 1, size=2))
            if (x, y) != pos and (x, y) != (spec.width - 2, spec.height - 2) and y < spec.height - 1:
                break
        g[y, x] = POOL_OBJECTS[int(r.integers(0, 3))]
        gs.append(g); ags.append(a)
    return np.stack(gs), np.stack(ags), None


#: per hook pool form: the scenario of hook_states.py whose start gets a twin, and what the twin's `aux` differs in
TWIN_SCENARIO = {"rbd_pool": 3, "lh_pool": 1, "rules_pool": 0, "lh12_pool": 1}


def hook_pool(form, K, r):
    """K hook-dense starts of the form's case of tests/hook_states.py, WITH their aux: K consecutive base states (env b of a case
    starts in scenario b % n: ten of them hold every scenario), the last replaced by a twin -- the cells and agent rows of one of
    the others with another `aux`: RedBlueDoors, the open blue door without the stale flag (what the grid shows is true); Locked-
    Hallway, the unlocked door's mask bit cleared; the rules, the success rule asking for the green ball.  Two envs on the pair are
    equal in everything but hook state, and step differently.  K = 1: one base state."""
    c = hs.case(HOOK_CASE[form])
    assert c.spec == SPECS[form], f"form {form} is not on the spec of {c.name}"
    lo = int(r.integers(0, hs.BASE - K))
    idx = lo + np.arange(K)
    g, a, x = (c.state[k][idx].copy() for k in ("grid", "agents", "aux"))
    if K > 1:
        j = int(np.flatnonzero(c.scenario[idx[:-1]] == TWIN_SCENARIO[form])[0])
        g[-1], a[-1], x[-1] = g[j], a[j], x[j]
        if form == "rbd_pool":
            assert x[j, 4] == 1 and g[j, x[j, 1], x[j, 0], 2] == hs.OPEN
            x[-1, 4] = 0
        elif form == "lh_pool":
            assert not x[j, 0] & 0x80 and x[j, 1], "an explicit aux with an unlocked door"
            x[-1, 1] = 0
        elif form == "lh12_pool":
            assert x[j, 0] & 0x80 and (x[j, 1] or x[j, 2]), "a geometric aux with an unlocked door"
            x[-1, 1:3] = 0
        else:
            x[-1] = layouts.rules_aux([("carries", hs.BALL, hs.GREEN, "success"), ("toggles_at", int(x[j, 7]), int(x[j, 8]), "failure", "open")])
            assert (x[-1] != x[j]).any() and (x[-1, 7:9] == x[j, 7:9]).all()
    return g, a, x


def pool_content(form, K, r):
    """the pool a `pool_refill` / `pool_replace` installs"""
    if form in HOOK_POOL_FORMS:
        return hook_pool(form, K, r)
    if form in ("pool4_objects", "big_objects1"):
        return object_pool(SPECS[form], K, int(r.integers(1, 1 << 30)))
    return small_pool(SPECS[form], K, r)


def make_env(form, B, device="cpu", backend=None, specialise=False):
    """One env of `form`; on the CPU over a SeqOracle (or `backend`), on a HIP device over the product's launcher.
    specialise: a HIP env steps on a kernel compiled for its shape at run time (env.specialise()); an oracle-backed one is as ever."""
    spec = SPECS[form]
    kw = {}
    if torch.device(device).type == "cpu":
        kw["backend"] = backend if backend is not None else SeqOracle(spec)
    env = BatchedMultiGridEnv(spec, B, device, first_env=FIRST_ENV.get(form, 0), **kw)
    if isinstance(env.backend, SeqOracle):
        env.backend.attach(env)
    if specialise and is_hip(env):
        env.specialise()
    if form in PLAIN_FORMS:
        st = util.random_state(spec, B, seed=7)
        env.load_state(st["grid"], st["agents"], st["rng"], None, st["step_count"])
    elif form in POOL1_FORMS:
        pg, pa = start_pool(spec)
        env.set_layout_pool(pg[1:2], pa[1:2])              # (one cell before the goal, facing it: both kinds of episode end)
        env.reset(seed=3)
    elif form == "pool_compact":
        pg, pa = start_pool(spec)
        env.set_layout_pool(pg, pa)
        env.reset(seed=3)
    elif form == "pool4_objects":
        g, a, _ = object_pool(spec, 4, 11)
        env.set_layout_pool(g, a)
        env.reset(seed=3)
    elif form == "bup_candidates":
        env.set_layout_generator("blockedunlockpickup", layout_seed=5, room_size=6, staged="candidates", lead=4)
        env.reset(seed=3)
        assert env._gen["stage"]["candidates"] == 4
    elif form in HOOK_POOL_FORMS:
        env.set_layout_pool(*hook_pool(form, POOL_K[form][0], np.random.default_rng(11)))
        env.reset(seed=3)
    elif form in ("rbd_candidates", "lh_candidates"):          # (one candidate per env: these generators never draw from np_random)
        env.set_layout_generator(form.split("_")[0].replace("rbd", "redbluedoors").replace("lh", "lockedhallway"), layout_seed=5,
                                 room_size=5 if form == "lh_candidates" else 0, staged="candidates", lead=4)
        env.reset(seed=3)
        assert env._gen["stage"]["candidates"] == 1 and env._gen["stage"]["aux"] is not None
    elif form == "playground_between":
        env.set_layout_generator("playground", layout_seed=5, room_size=7, lead=4)     # (staged=True, the default: it must fall back)
        env.reset(seed=3)
        st = env._gen["stage"]
        assert not st.get("candidates") and st["external"] == 2 and st["lead"] == 4, "Playground did not fall back to 'between'"
    else:
        staged = {"gen": False, "gen_candidates": "candidates", "gen_between": "between"}[form]
        env.set_layout_generator("empty_random", layout_seed=5, staged=staged, lead=4)
        env.reset(seed=3)
        assert (env._gen.get("stage") is None) == (form == "gen")
    return env


# ---- the call list ------------------------------------------------------------------------------------------------------------------

def legal_kinds(form, B, gpu):
    """every kind `form` can meet at batch B (what the census asks for)"""
    kinds = ["step", "rollout", "snapshot", "snapshot_out", "restore", "fork", "edit", "load_state_dict", "track", "reset_totals",
             "stats_lsd", "seed", "gen_obs", "full_obs", "one_hot_obs", "step_one_hot"]
    if form not in PLAIN_FORMS:
        kinds += ["reset_done", "reset"]
    if form in POOL_FORMS:
        kinds += ["pool_refill", "pool_replace"]
    if B >= 128:
        kinds.append("split")
    if gpu:
        kinds += ["capture_replay", "graph_again"]
        if form in POOL_FORMS or form in PLAIN_FORMS:
            kinds.append("persistent")
        if B >= 128:
            kinds.append("step_chains")
    return kinds


def legal_query_kinds(form, B, gpu):
    """every query kind `form` can meet at batch B: `_copy_entry` admits a query wherever the list stands between two calls (no session
    is open there, a state is loaded, the env is no sub-shard)"""
    return list(QUERY_KINDS[:-2]) + (list(GPU_QUERY_KINDS) if gpu else [])


def without_queries(ops):
    return [o for o in ops if o["kind"] not in QUERY_KINDS]


def make_ops(form, B, n_ops, seed, gpu=False, stretch=None, weights=None, kinds=None, every_third=None, queries=False):
    """The whole list of calls of one sequence.

    gpu          the GPU-only kinds are in
    stretch      (s, e): call s is `tm_begin` (a snapshot of the whole batch, the kept ones forgotten), and the calls s+1 .. e-1 are
                 PURE_KINDS that use only snapshots taken after s -- what the time machine records, restores and repeats
    kinds        restrict the kinds drawn (the large-batch test); every_third: that call at every third index instead of a draw
    queries      the query layer: zero to two QUERY_KINDS behind every call, drawn from a generator of their own (`rq`), so that
                 `without_queries()` of the list is the list of queries=False, arguments included; n_ops, `stretch` and every_third
                 count the other calls.  A `step_chains` directly in front of a query that goes through the env's `_row_set` is
                 not joined by apply(): the query carries first_consumer=True, and its own join() is what orders it behind the
                 chains.
    The RedBlueDoors and LockedHallway forms (ORDER_FORMS): step, step_one_hot, step_chains, split, capture_replay and graph_again
    carry a `hook_order` -- present about half the time, None otherwise --, drawn from a third generator (`rh`): step(hook_order=...)
    leaves the bound hot path for the slow entry, with its marker bookkeeping, generator launches and accounting launch.  rollout
    and persistent have no such parameter."""
    r = np.random.default_rng([seed, B, SEED_ORDER.index(form)])
    rq = np.random.default_rng([seed, B, SEED_ORDER.index(form), 1])
    rh = np.random.default_rng([seed, B, SEED_ORDER.index(form), 2])
    spec = SPECS[form]
    A, H, W = spec.num_agents, spec.height, spec.width
    source = form not in PLAIN_FORMS
    w = dict(WEIGHTS, **QUERY_WEIGHTS)
    w.update(weights or {})
    allowed = set(legal_kinds(form, B, gpu) + legal_query_kinds(form, B, gpu)) if kinds is None else set(kinds)
    S = {"tracking": None, "snaps": {}, "graphs": {}, "version": 0, "persistent": 0, "K": POOL_K.get(form, (0,))[0], "next_slot": 0,
         "next_graph": 0, "staged": form in STAGED_FORMS,
         # (what the query layer keeps, from the calls' arguments alone: no draw of `r` depends on it)
         "epoch": 0, "touched": np.zeros(B, bool), "qgraphs": {}, "next_qgraph": 0, "last_table_ids": None}

    def actions(*lead):
        a = r.integers(0, 7, size=lead + (B, A)).astype(np.int8)
        a[r.random(lead + (B, A)) < 0.25] = 2                 # forward: episodes end by reaching something, too
        if form in HOOK_POOL_FORMS:                           # (the starts stand in front of what their hook is about: toggle, pick up)
            key = r.choice([5, 3], size=a.shape).astype(np.int8) if form == "rules_pool" else np.int8(5)
            a = np.where(r.random(a.shape) < 0.35, key, a)
        return a

    def auto():
        return bool(source and r.random() < 0.75)

    def ids(n=None, distinct=True):
        n = int(r.integers(1, min(B, 40) + 1)) if n is None else n
        return (r.permutation(B)[:n] if distinct else r.integers(0, B, size=n)).astype(np.int64)

    def usable(in_stretch):
        return [s for s, v in S["snaps"].items() if not in_stretch or v["pure"]]

    def draw(kind, pure):
        op = {"kind": kind}
        tracked = S["tracking"] is not None
        if kind in ("step", "step_chains"):
            op.update(acts=actions(), auto_reset=auto())
        elif kind == "step_one_hot":
            op.update(acts=actions(), auto_reset=bool(form in POOL1_FORMS + ("pool4_objects",) and r.random() < 0.5))
        elif kind == "rollout":
            op.update(acts=actions(int(r.integers(1, 5))), auto_reset=auto())
        elif kind == "reset":
            mask = None
            if r.random() < 0.8:
                mask = r.random(B) < r.choice([0.1, 0.5, 0.9])
                mask = mask if r.random() < 0.5 else mask.astype(np.uint8)
            op.update(seed=int(r.integers(0, 1000)) if r.random() < 0.5 else None, mask=mask)
        elif kind == "snapshot":
            e = None if r.random() < 0.4 else ids(distinct=bool(r.random() < 0.7))
            slot = S["next_slot"]
            S["next_slot"] = (slot + 1) % MAX_SNAPS
            S["snaps"][slot] = {"rows": B if e is None else len(e), "tracked": tracked, "pure": pure, "all": e is None, "epoch": S["epoch"]}
            op.update(slot=slot, env_ids=e)
        elif kind == "snapshot_out":
            fit = [s for s in usable(pure) if S["snaps"][s]["tracked"] == tracked]
            if not fit:
                return None
            slot = int(r.choice(fit))
            v = S["snaps"][slot]
            e = None if v["all"] and r.random() < 0.5 else ids(v["rows"])
            v.update(pure=pure, all=v["all"] and e is None, epoch=S["epoch"])
            op.update(slot=slot, env_ids=e)
        elif kind == "restore":
            have = usable(pure)
            if not have:
                return None
            bare = [s for s in have if tracked and not S["snaps"][s]["tracked"]]
            slot = int(r.choice(bare if bare and r.random() < 0.5 else have))   # (rows without the running episode, into a tracking env)
            n_s = S["snaps"][slot]["rows"]
            if r.random() < 0.25:
                e, rows = None, (None if n_s >= B and r.random() < 0.5 else r.integers(0, n_s, size=B).astype(np.int64))
            else:
                e = ids()
                rows = None if len(e) <= n_s and r.random() < 0.3 else r.integers(0, n_s, size=len(e)).astype(np.int64)
            op.update(slot=slot, env_ids=e, rows=rows, check=bool(r.random() < 0.3),
                      repeated=rows is not None and len(np.unique(rows)) < len(rows), carries=S["snaps"][slot]["tracked"])
        elif kind == "fork":
            n = int(r.integers(1, min(B, 8) + 1))
            src, dst = ids(n, distinct=False), ids(n)
            if n > 1 and r.random() < 0.6 and src[-1] not in dst[1:]:
                dst[0] = src[-1]                              # a destination that is somebody's source hands on its OLD state
            op.update(src=src, dst=dst, check=bool(r.random() < 0.3))
        elif kind == "edit":
            big = B >= 1024         # (the large batch: a sixteenth of the envs, never empty on empty, near the Empty start -- in view)
            triple = EDIT_CELLS[int(r.integers(1 if big else 0, len(EDIT_CELLS)))]
            op.update(env_ids=ids(B // 16 if big else int(r.integers(1, min(B, 6) + 1))), y=int(r.integers(1, 5 if big else H - 1)),
                      x=int(r.integers(1, 6 if big else W - 1)), value=int(layouts.pack_cells_for(spec, triple[None])[0]), triple=triple)
        elif kind == "load_state_dict":
            if form in GEN_FORMS:
                S["version"] += 1
                S["staged"] = True                            # (set_layout_generator's default: an unstaged generator comes back staged)
        elif kind in ("pool_refill", "pool_replace"):
            if kind == "pool_replace":
                ks = POOL_K[form]
                S["K"] = ks[1 - ks.index(S["K"])]
                S["version"] += 1
            g, a, x = pool_content(form, S["K"], r)
            op.update(grids=g, agents=a, aux=x)
        elif kind == "track":
            if not tracked and r.random() < 0.5:              # (half of a run without the accounting: the kinds that refuse it)
                return None
            value = [False, True, None, None][int(r.integers(0, 4))] if tracked else [False, True][int(r.integers(0, 2))]
            S["tracking"] = value
            S["version"] += 1
            op.update(value=value)
        elif kind in ("reset_totals", "stats_lsd"):
            if not tracked:
                return None
        elif kind == "seed":
            op.update(seed=int(r.integers(0, 1000)))
        elif kind == "gen_obs":
            op.update(one_hot=bool(r.random() < 0.5))
        elif kind == "split":
            op.update(acts=actions(3), steps=r.integers(1, 4, size=2), auto_reset=auto())
        elif kind == "capture_replay":
            T = int(r.integers(1, 4))
            keep = not pure and r.random() < 0.8
            op.update(acts=actions(T), auto_reset=auto(), sub_shards=int(r.integers(1, 3)) if B >= 128 else 1, keep=None)
            if keep:
                op["keep"] = S["next_graph"]
                S["graphs"][S["next_graph"]] = {"version": S["version"], "acts": op["acts"], "auto_reset": op["auto_reset"]}
                S["next_graph"] += 1
        elif kind == "graph_again":
            live = [g for g, v in S["graphs"].items() if v["version"] == S["version"]]
            if not live:
                return None
            g = int(r.choice(live))
            op.update(graph=g, acts=S["graphs"][g]["acts"], auto_reset=S["graphs"][g]["auto_reset"])
        elif kind == "persistent":
            if tracked or S["persistent"] >= 2:
                return None
            S["persistent"] += 1
            op.update(acts=actions(int(r.integers(2, 4))), auto_reset=bool(form in POOL_FORMS and r.random() < 0.7))
        if kind == "step_chains" and tracked:
            return None
        return op

    # ---- the query layer: every draw below is one of `rq`
    def q_ids(rows=B):
        """row indices of a query: 1..MAX_QUERY_ROWS of them, repeated half the time; now and then None (every row, in order)"""
        if rows <= 160 and rq.random() < 0.05:  # (the whole of a small batch or snapshot; never of the large batch)
            return None
        n = int(rq.integers(1, min(rows, MAX_QUERY_ROWS) + 1))
        return (rq.integers(0, rows, size=n) if rq.random() < 0.5 else rq.permutation(rows)[:n]).astype(np.int64)

    def q_subset(values, lo=1):
        values = list(values)
        n = int(rq.integers(lo, len(values) + 1))
        return sorted(int(v) for v in rq.permutation(values)[:n])

    def q_args(which, n):
        """the keyword arguments of one row query over n output rows"""
        if which == "key":
            return {"salt": SALTS[int(rq.integers(0, 2))], "step_count": bool(rq.random() < 0.5), "rng": bool(rq.random() < 0.5)}
        if which == "mask":
            return {"expand": bool(rq.random() < 0.5)}
        q = {"field": bool(rq.random() < 0.35), "types": None, "colors": None, "agents": None, "points": None,
             "through": tuple(t for t in THROUGH if rq.random() < 0.5), "avoid_lava": bool(rq.random() < 0.4)}
        mode = int(rq.integers(0, 6))
        if mode in (0, 1, 4):
            q["types"] = q_subset(SOURCE_TYPES)[:3]
        if mode == 1:
            q["colors"] = q_subset(range(6))[:3]
        if mode in (2, 4):
            q["agents"] = q_subset(range(A))
        if mode in (3, 5) or rq.random() < 0.15:
            # (x, y) per output row, some outside the grid; every third row has none inside: a row without a source
            P = int(rq.integers(1, 4))
            pts = np.stack([rq.integers(-2, W + 2, size=(n, P)), rq.integers(-2, H + 2, size=(n, P))], axis=-1).astype(np.int16)
            pts[rq.random(n) < 0.33] = (W + 1, -1)
            q["points"] = pts
        return q

    def draw_query(kind, pure, chained, fresh=False):
        op = {"kind": kind}
        if kind in ROW_QUERIES:
            e = q_ids()
            op.update(ids=e, keep_out=bool(rq.random() < 0.5), **q_args(kind[2:].split("_")[-1], B if e is None else len(e)))
        elif kind == "q_snap":
            have = usable(pure)
            if not have:
                return None
            stale = [s for s in have if S["snaps"][s]["epoch"] < S["epoch"]]
            slot = int(rq.choice(stale if stale and rq.random() < 0.5 else have))
            v = S["snaps"][slot]
            e = q_ids(v["rows"])
            which = ("key", "mask", "distance")[int(rq.integers(0, 3))]
            op.update(slot=slot, ids=e, which=which, keep_out=bool(rq.random() < 0.5), stale=v["epoch"] < S["epoch"],
                      **q_args(which, v["rows"] if e is None else len(e)))
        elif kind == "q_table":
            e = q_ids()
            e = np.arange(min(B, MAX_QUERY_ROWS), dtype=np.int64) if e is None else e
            last = S["last_table_ids"]
            if last is not None and rq.random() < 0.6:          # (envs the table may know: half of the last call's)
                e = np.concatenate([last[:(len(last) + 1) // 2], e])[:MAX_QUERY_ROWS] if B > MAX_QUERY_ROWS else e
            S["last_table_ids"] = e
            op.update(ids=e, mode="insert" if rq.random() < 0.6 else "lookup", count=bool(rq.random() < 0.5))
        elif kind == "q_select":
            op.update(type=COMMON_TYPE[form], k=("one", "less", "all", "more", "pad")[int(rq.integers(0, 5))],
                      values=bool(rq.random() < 0.5), fill=(-1, 12345)[int(rq.integers(0, 2))], keep_out=bool(rq.random() < 0.5))
        elif kind == "q_graph":
            n = int(rq.integers(1, min(B, MAX_QUERY_ROWS) + 1))
            g = S["next_qgraph"] % MAX_QUERY_GRAPHS
            S["next_qgraph"] += 1
            op.update(graph=g, ids=rq.integers(0, B, size=n).astype(np.int64), type=COMMON_TYPE[form], k=int(rq.integers(1, n * A + 3)),
                      salt=SALTS[int(rq.integers(0, 2))], step_count=bool(rq.random() < 0.5), rng=bool(rq.random() < 0.5),
                      through=tuple(t for t in THROUGH if rq.random() < 0.5), avoid_lava=bool(rq.random() < 0.4))
            S["qgraphs"][g] = {"version": S["version"], "op": op}
        elif kind == "q_graph_again":
            live = [g for g, v in S["qgraphs"].items() if v["version"] == S["version"]]
            if not live:
                return None
            op = dict(S["qgraphs"][int(rq.choice(live))]["op"], kind="q_graph_again")
        if kind == "q_action_mask" and form in RBD_FORMS and rq.random() < 0.5:
            op["ids"] = None      # (every row: the few envs whose stale door has a live agent in front of it are among them)
        if fresh:                 # (every row, and a key without np_random -- the words differ from env to env: what can be equal is)
            op.update(ids=None, rng=False)
        if kind in ROW_QUERIES:
            e = op["ids"]
            op["hits_touched"] = bool(S["touched"].all() if e is None else S["touched"][e].any())
            S["touched"][...] = False
        if chained:
            op["first_consumer"] = True
        return op

    def draw_queries(prev, pure):
        """zero to two queries behind `prev`; behind a step_chains at least one, and that one through the env's `_row_set`"""
        if not queries:
            return []
        chained = prev["kind"] == "step_chains"
        # a hook pool form behind a reset(): the envs just restarted stand on their starts, those on a start and on its twin (hook_pool)
        # equal in everything but aux -- the first query is a state_key of the whole batch
        fresh = form in HOOK_POOL_FORMS and prev["kind"] == "reset" and "q_state_key" in allowed
        n = max(int(rq.choice(3, p=QUERY_COUNT_P)), 1 if chained or fresh else 0)
        out = []
        for j in range(n):
            if fresh and j == 0:
                out.append(draw_query("q_state_key", pure, False, fresh=True))
                qran["q_state_key"] = qran.get("q_state_key", 0) + 1
                continue
            first = chained and j == 0
            names = sorted(k for k in allowed if k in QUERY_KINDS and (not pure or k in PURE_KINDS)
                           and (not first or k in (FIRST_CONSUMERS if not pure else ROW_QUERIES + ("q_select",))))
            if not names:
                break
            p = np.array([w[k] * (4 if qran.get(k, 0) < 2 else 1) for k in names], float)
            for _ in range(8):                               # (a kind with nothing to work on -- no snapshot, no graph -- gives way)
                op = draw_query(names[int(rq.choice(len(names), p=p / p.sum()))], pure, first)
                if op is not None:
                    qran[op["kind"]] = qran.get(op["kind"], 0) + 1
                    out.append(op)
                    break
        return out

    def note(op):
        """what the query layer remembers of a call: which envs it restored, reset or edited, and that the pool or the state changed
        under the kept snapshots (the calls' arguments alone)"""
        k = op["kind"]
        if k in ("load_state_dict", "pool_refill", "pool_replace"):
            S["epoch"] += 1
        if k == "restore":
            S["touched"][op["env_ids"] if op["env_ids"] is not None else slice(None)] = True
        elif k == "reset":
            S["touched"][op["mask"].astype(bool) if op["mask"] is not None else slice(None)] = True
        elif k == "edit":
            S["touched"][op["env_ids"]] = True
        elif k == "fork":
            S["touched"][op["dst"]] = True

    def main_op(i, pure):
        if stretch is not None and i == stretch[0]:
            S["snaps"] = {}
            return {"kind": "tm_begin"}
        if every_third is not None and i % 3 == 2:
            return {"kind": "step", "acts": actions(), "auto_reset": True}
        if every_third is not None and i % 9 == 3:           # (an edit right behind a step whose restarts marked their envs)
            return draw("edit", pure)
        if pure and i == stretch[0] + 3:                     # (so that the stretch has a snapshot of its own to restore and fork from)
            return draw("snapshot", pure)
        names = sorted(k for k in allowed if k not in QUERY_KINDS and (not pure or k in PURE_KINDS))
        # (a kind the list has met less than twice is four times as likely: every list holds every kind its form allows)
        p = np.array([w[k] * (4 if ran.get(k, 0) < 2 else 1) for k in names], float)
        while True:
            op = draw(names[int(r.choice(len(names), p=p / p.sum()))], pure)
            if op is not None:
                break
        ran[op["kind"]] = ran.get(op["kind"], 0) + 1
        return op

    def with_order(op):
        """the visiting order of a stepping call of an ORDER_FORMS form: u8[B,A] (or [T,B,A]) permutations, or None -- every draw is
        one of `rh`, and no other form's call gets the key"""
        def order(*lead):
            if rh.random() < 0.5:
                return None
            return np.argsort(rh.random(lead + (B, A)), axis=-1).astype(np.uint8)
        k = op["kind"]
        if k in ("step", "step_one_hot", "step_chains"):
            op["hook_order"] = order()
        elif k in ("capture_replay", "split"):
            op["hook_order"] = order(op["acts"].shape[0])
            if k == "capture_replay" and op["keep"] is not None:
                S["graphs"][op["keep"]]["hook_order"] = op["hook_order"]
        elif k == "graph_again":                              # (the graph reads the order it was captured with)
            op["hook_order"] = S["graphs"][op["graph"]]["hook_order"]

    ops, ran, qran = [], {}, {}
    for i in range(n_ops):
        pure = stretch is not None and stretch[0] < i < stretch[1]
        op = main_op(i, pure)
        if form in ORDER_FORMS:
            with_order(op)
        ops.append(op)
        note(op)
        ops.extend(draw_queries(op, pure or op["kind"] == "tm_begin"))     # (behind the snapshot: part of what is repeated)
    return ops


def describe(op) -> str:
    parts = []
    for k, v in op.items():
        if k in ("kind", "triple"):
            continue
        if isinstance(v, np.ndarray):
            v = v.tolist() if v.size <= 8 else f"{v.dtype}{list(v.shape)}"
        parts.append(f"{k}={v}")
    return f"{op['kind']}({', '.join(parts)})"


# ---- performing a call --------------------------------------------------------------------------------------------------------------

def new_ctx():
    return {"snaps": {}, "graphs": {}, "tm": None, "outs": {}, "table": None, "selector": None, "qgraphs": {}, "warm_table": None,
            "seen": {}}                                        # (seen: what apply() itself met, on either kind of env)


def is_hip(env) -> bool:
    return getattr(env.backend, "name", "") == "hip"


def apply(env, op, ctx, nxt=None) -> dict:
    """`perform()`, and what two envs that share a fault of the host logic cannot show each other: a stepping call's visiting order
    reached every launch it stands for (an oracle-backed env: the launcher counts them), and a pool call installed the aux it was
    given."""
    be = env.backend
    ho, before = op.get("hook_order"), getattr(be, "ordered_launches", None)
    outs = perform(env, op, ctx, nxt)
    if ho is not None and before is not None:
        k = op["kind"]
        want = {"capture_replay": 2 * len(op["acts"]), "graph_again": len(op["acts"]), "split": int(np.sum(op.get("steps", 0)))}.get(k, 1)
        assert be.ordered_launches - before == want, \
            f"{describe(op)}: {be.ordered_launches - before} launch(es) got the visiting order, {want} stand for the call"
    if op["kind"] in ("pool_refill", "pool_replace"):
        pool = env._pool
        assert (pool[2] is None) == (op["aux"] is None), f"{describe(op)}: the pool's aux"
        assert torch.equal(pool[0].cpu(), torch.from_numpy(layouts.pack_cells_for(env.spec, op["grids"]))) \
            and torch.equal(pool[1].cpu(), torch.from_numpy(op["agents"])) \
            and (pool[2] is None or torch.equal(pool[2].cpu(), torch.from_numpy(op["aux"]))), \
            f"{describe(op)}: the pool does not hold the layouts, agent rows and aux it was given"
    return outs


def perform(env, op, ctx, nxt=None) -> dict:
    """One call on `env`.  Returns what the call wrote or handed back that is not part of the env state: name -> tensor (the env's
    own output buffers by name, a rollout's dict and a query's answers under 'out.<key>').  nxt: the call that follows in the list
    (`following`), which decides the shape of a step_chains."""
    dev, kind, hip = env.device, op["kind"], is_hip(env)
    be = env.backend

    def dv(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def outputs(auto_reset=False, one_hot=False):
        names = (("_one_hot",) if one_hot else ("obs",)) + OUTPUTS[1:] + (("was_reset",) if auto_reset else ())
        return {n: getattr(env, n) for n in names}

    def steps(acts, auto_reset, times=1, order=None):
        for _ in range(times):
            for t in range(acts.shape[0]):
                env.step(dv(acts[t]), auto_reset=auto_reset, hook_order=None if order is None else dv(order[t]))
        return outputs(auto_reset)

    ho = op.get("hook_order")                                  # (a stepping call of the ORDER_FORMS: u8[B,A], u8[T,B,A] or None)
    if ho is not None and env._mark["armed"]:
        ctx["seen"]["stepped_with_hook_order_while_armed"] = ctx["seen"].get("stepped_with_hook_order_while_armed", 0) + 1
        if isinstance(be, SeqOracle):
            be._count("stepped_with_hook_order_while_armed")
    if kind == "step":
        env.step(dv(op["acts"]), auto_reset=op["auto_reset"], hook_order=dv(ho))
        return outputs(op["auto_reset"])
    if kind == "step_one_hot":
        env.step(dv(op["acts"]), auto_reset=op["auto_reset"], one_hot=True, hook_order=dv(ho))
        return outputs(op["auto_reset"], one_hot=True)
    if kind == "rollout":
        return {"out." + k: v for k, v in env.rollout(dv(op["acts"]), auto_reset=op["auto_reset"]).items()}
    if kind == "reset_done":
        return {"was_reset": env.reset_done()}
    if kind == "reset":
        env.reset(seed=op["seed"], mask=dv(op["mask"]))
        return {"obs": env.obs, "dir": env.dir, "was_reset": env.was_reset}
    if kind == "tm_begin":
        ctx["snaps"] = {}
        ctx["tm"] = env.snapshot()
        return {}
    if kind == "snapshot":
        ctx["snaps"][op["slot"]] = env.snapshot(dv(op["env_ids"]))
        return {}
    if kind == "snapshot_out":
        snap = ctx["snaps"][op["slot"]]
        assert env.snapshot(dv(op["env_ids"]), out=snap) is snap
        return {}
    if kind == "restore":
        env.restore(ctx["snaps"][op["slot"]], dv(op["env_ids"]), dv(op["rows"]), check=op["check"])
        return {}
    if kind == "fork":
        if isinstance(be, SeqOracle):
            be.forking = True
        env.fork(dv(op["src"]), dv(op["dst"]), check=op["check"])
        if isinstance(be, SeqOracle):
            be.forking = False
        return {}
    if kind == "edit":
        cells = env.cells                                      # (the public tensor: handing it out takes the marker's promise back)
        if env.spec.cell_bytes == 3:
            cells[dv(op["env_ids"]), op["y"], op["x"]] = dv(op["triple"])
        else:
            cells[dv(op["env_ids"]), op["y"], op["x"]] = op["value"]
        return {}
    if kind == "load_state_dict":
        env.load_state_dict(env.state_dict())
        if isinstance(be, SeqOracle) and be.shadow is not None:          # (load_state: every env restarts, the finished ones stay out)
            model_restart(be.shadow, None)
            be.shadow["over"][...] = env.is_done().numpy()
        return {}
    if kind in ("pool_refill", "pool_replace"):
        env.set_layout_pool(op["grids"], op["agents"], op["aux"])
        return {}
    if kind == "track":
        env.track_episodes(op["value"])
        if isinstance(be, SeqOracle):
            be.shadow = None
            if op["value"] is not None:
                be.shadow = new_state(env.batch, env.spec.num_agents)
                be.shadow["over"][...] = env.is_done().numpy()
        return {}
    if kind == "reset_totals":
        env.episode_stats.reset_totals()
        if isinstance(be, SeqOracle):
            for n in ("sum_return", "sum_length", "counts"):
                be.shadow[n][...] = 0
        return {}
    if kind == "stats_lsd":
        env.episode_stats.load_state_dict(env.episode_stats.state_dict())
        return {}
    if kind == "seed":
        env.seed(op["seed"])
        return {}
    if kind == "gen_obs":
        obs, dirs = env.gen_obs(one_hot=op["one_hot"])
        return {"_one_hot" if op["one_hot"] else "obs": obs, "dir": dirs}
    if kind == "full_obs":
        return {"_full": env.full_obs()}
    if kind == "one_hot_obs":
        return {"_one_hot": env.one_hot_obs()}
    if kind == "split":
        children = env.split(2)
        assert len(children) == 2
        for c, n in zip(children, op["steps"]):
            lo, hi = c._range
            for t in range(int(n)):
                c.step(dv(op["acts"][t, lo:hi]), auto_reset=op["auto_reset"], hook_order=None if ho is None else dv(ho[t, lo:hi]))
                invariants(c, f"sub-shard [{lo}, {hi}) step {t}")
        return outputs(op["auto_reset"])
    # ---- the GPU-only kinds, and what they are on the oracle
    if kind == "capture_replay":
        if not hip:
            if op["keep"] is not None:
                ctx["graphs"][op["keep"]] = True
            return steps(op["acts"], op["auto_reset"], times=2, order=ho)
        graph = env.capture_steps(dv(op["acts"]), auto_reset=op["auto_reset"], sub_shards=op["sub_shards"], hook_order=dv(ho))
        graph.replay(); graph.replay()
        if op["keep"] is not None:
            ctx["graphs"][op["keep"]] = graph
        return outputs(op["auto_reset"])
    if kind == "graph_again":
        if not hip:
            return steps(op["acts"], op["auto_reset"], order=ho)
        ctx["graphs"][op["graph"]].replay()
        return outputs(op["auto_reset"])
    if kind == "persistent":
        if not hip:
            return steps(op["acts"], op["auto_reset"])
        acts = dv(op["acts"])
        with env.persistent(max_steps=acts.shape[0], auto_reset=op["auto_reset"]) as ps:
            for t in range(acts.shape[0]):
                ps.step(acts[t])
        return outputs(op["auto_reset"])
    if kind == "step_chains":
        if not hip:
            return steps(op["acts"][None], op["auto_reset"], order=None if ho is None else ho[None])
        env.step(dv(op["acts"]), auto_reset=op["auto_reset"], sub_shards=2, hook_order=dv(ho))
        if unjoined(op, nxt):                                  # (the query that follows joins: nothing may read this env before it)
            return {}
        env.join()
        return outputs(op["auto_reset"])
    if kind in QUERY_KINDS:
        outs = apply_query(env, op, ctx)
        if op.get("first_consumer"):                           # (behind the query's join(): what the unjoined step handed back)
            outs.update({n: getattr(env, n) for n in OUTPUTS})
        return outs
    raise ValueError(f"unknown call kind {kind!r}")


def unjoined(op, nxt) -> bool:
    """`op` is a step_chains whose join() is left to the query `nxt` that follows it (on the HIP env: nothing may read the env in between)"""
    return op["kind"] == "step_chains" and nxt is not None and bool(nxt.get("first_consumer"))


def following(ops, i):
    return ops[i + 1] if i + 1 < len(ops) else None


WHICH = {"q_state_key": "key", "q_action_mask": "mask", "q_distance": "distance"}


def apply_query(env, op, ctx) -> dict:
    """One call of the query layer on `env`: what it answered, under 'out.<name>' keys.  On an oracle-backed env the answers also feed
    the census (what a query met can only be seen in its answer)."""
    dev, kind = env.device, op["kind"]
    be, sp = env.backend, env.spec
    A, H, W = sp.num_agents, sp.height, sp.width
    seen = be._count if isinstance(be, SeqOracle) else (lambda what, n=1: None)

    def dv(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def kept(name, shape, dtype, fill):
        """the tensor this context keeps for out= of that name and shape"""
        key = (name,) + tuple(shape)
        if key not in ctx["outs"]:
            ctx["outs"][key] = torch.full(tuple(shape), fill, dtype=dtype, device=dev)
        return ctx["outs"][key]

    def row_query(target, which, a, n_rows):
        idx = dv(a["ids"])
        n = n_rows if idx is None else int(idx.shape[0])
        keep = a.get("keep_out", False)
        t = None
        if isinstance(be, SeqOracle) and sp.env_kind in HOOK_KINDS:     # (the rows the query names, for the census of what it met)
            t = target.tensors if target is not env else {"cells": env._cells, "agents": env.agents, "rng": env.rng,
                                                           "step_count": env.step_count, "aux": env.aux}
            t = {m: (v if idx is None else v[idx]).numpy() for m, v in t.items() if m in ("cells", "agents", "rng", "step_count", "aux")}
        if which == "key":
            out = kept("key", (n,), torch.int64, 0) if keep else None
            res = target.state_key(idx, salt=a["salt"], step_count=a["step_count"], rng=a["rng"], out=out)
            if t is not None:
                # two rows equal in cells, agents and whatever else the key covers, but for `aux`: their keys must differ
                first = {}
                for i in range(n):
                    rest = t["cells"][i].tobytes() + t["agents"][i].tobytes() + (t["step_count"][i].tobytes() if a["step_count"] else b"") \
                        + (t["rng"][i].tobytes() if a["rng"] else b"")
                    j = first.setdefault(rest, i)
                    if t["aux"][j].tobytes() != t["aux"][i].tobytes():
                        assert int(res[i]) != int(res[j]), f"rows {j} and {i} differ in hook state only, and have one state key"
                        seen("state_keys_differ_by_hook_state_only")
            return res
        if which == "mask":
            shape, dt = ((n, A, 7), torch.bool) if a["expand"] else ((n, A), torch.uint8)
            res = target.action_mask(idx, expand=a["expand"], out=kept("mask", shape, dt, 0) if keep else None)
            if isinstance(be, SeqOracle):
                bits = res[..., 2:6] if a["expand"] else ((res[..., None].to(torch.int32) >> torch.arange(2, 6)) & 1).bool()
                seen("mask_with_a_clear_and_a_set_bit_beyond_the_turns", int(bool(bits.any()) and not bool(bits.all())))
            if t is not None and sp.env_kind == "redbluedoors":
                # a live agent in front of the blue door while the stale flag is up: the door's object is closed, whatever the
                # grid shows there (a failed opening, an edit over the door)
                d = t["agents"][..., 1] & 3
                fx, fy = t["agents"][..., 2] + np.array([1, 0, -1, 0])[d], t["agents"][..., 3] + np.array([0, 1, 0, -1])[d]
                at = (t["agents"][..., 4] == 0) & (fx == t["aux"][:, None, 0]) & (fy == t["aux"][:, None, 1])
                seen("mask_of_a_stale_door", int(((t["aux"][:, 4] == 1) & at.any(axis=1)).sum()))
            return res
        field = a["field"]
        out = kept("dist", (n, H, W) if field else (n, A), torch.int16, -1) if keep else None
        res = (target.distance_field if field else target.agent_distance)(
            idx, types=a["types"], colors=a["colors"], agents=a["agents"], points=dv(a["points"]), through=a["through"],
            avoid_lava=a["avoid_lava"], out=out)
        if isinstance(be, SeqOracle) and not field and bool((res < 0).any()) and bool((res >= 0).any()):
            seen("agent_distance_with_and_without_a_way")
        if t is not None and sp.env_kind == "lockedhallway":      # (doors that the agents' keys have opened, or a start shows open)
            g3 = layouts.unpack_cells_for(sp, t["cells"])
            seen("distance_over_a_grid_with_an_open_door", int(((g3[..., 0] == hs.DOOR) & (g3[..., 2] == hs.OPEN)).any(axis=(1, 2)).sum()))
        return res

    def table():
        if ctx.get("table") is None:
            ctx["table"] = env.key_table(TABLE_CAPACITY)
        return ctx["table"]

    def selector():
        if ctx.get("selector") is None:
            ctx["selector"] = env.selector(max(min(env.batch, SELECT_MAX), MAX_QUERY_ROWS * A))
        return ctx["selector"]

    if kind in ROW_QUERIES:
        return {"out." + WHICH[kind]: row_query(env, WHICH[kind], op, env.batch)}
    if kind == "q_obs_key":
        return {"out.obs_key": env.obs_key()}
    if kind == "q_snap":
        snap = ctx["snaps"][op["slot"]]
        return {"out.snap_" + op["which"]: row_query(snap, op["which"], op, snap.rows)}
    if kind == "q_table":
        keys = env.state_key(dv(op["ids"]))
        t = table()
        if op["mode"] == "insert":
            res = t.insert(keys, first=True, visits=True, count=op["count"])
            outs = {"out.is_new": res.is_new, "out.first": res.first, "out.visits": res.visits}
            if isinstance(be, SeqOracle):
                known = ~res.is_new & (res.first == torch.arange(keys.numel()))       # (the first holder of a key the table had)
                if bool(res.is_new.any()) and bool(known.any()):
                    seen("insert_of_new_and_known_keys")
        else:
            res = t.lookup(keys, visits=True)
            outs = {"out.held": res.entry >= 0, "out.visits": res.visits}
            seen("lookup_with_a_miss", int(isinstance(be, SeqOracle) and bool((res.entry < 0).any())))
        # (what include/mgx.h promises whatever the placement: not the entry ids)
        outs["out.entries"] = torch.tensor([t.entries(), t.dropped()], dtype=torch.int64)
        return outs
    if kind == "q_select":
        n = min(env.batch, SELECT_MAX)
        ids = None if n == env.batch else torch.arange(n, device=dev)
        dist = env.agent_distance(ids, types=[op["type"]])        # (first: its join() is what may order the rest behind the chains)
        score = dist[:, 0].to(torch.int32).contiguous()
        keep = env.agents[:n, 0, 4] == 0
        cand = int(keep.sum())
        k = max(1, {"one": 1, "less": cand - 1, "all": cand, "more": cand + 1, "pad": env.batch + 9}[op["k"]])
        values = torch.arange(n, device=dev) * 3 + 1 if op["values"] else None
        out = Selection(kept("index", (k,), torch.int64, 0), kept("count", (2,), torch.int32, 0)) if op["keep_out"] else None
        res = selector().select(score, keep, k=k, values=values, fill=op["fill"], out=out)
        if isinstance(be, SeqOracle) and cand:
            if k < cand:
                T, quota, tied, _ = threshold(score.numpy(), keep.numpy(), k)
                seen("select_cut_inside_a_tie", int(tied > quota))
            seen("select_padded", int(k > cand))
        return {"out.index": res.index, "out.count": res.count, "out.score": score}
    if kind in GPU_QUERY_KINDS:
        return query_graph(env, op, ctx, table(), selector())
    raise ValueError(f"unknown query kind {kind!r}")


def query_graph(env, op, ctx, table, selector) -> dict:
    """q_graph: state_key + action_mask + agent_distance + table.insert(count=False) + select of one set of rows, captured into one
    torch.cuda.graph and replayed once (the graph is kept in its slot); q_graph_again: that graph replayed.  The oracle-backed env
    makes the same calls eagerly, both times."""
    dev, A = env.device, env.spec.num_agents
    idx = torch.from_numpy(op["ids"]).to(dev)
    n = int(idx.shape[0])

    def buffers():
        return {"keys": torch.zeros(n, dtype=torch.int64, device=dev), "mask": torch.zeros((n, A), dtype=torch.uint8, device=dev),
                "dist": torch.full((n, A), -1, dtype=torch.int16, device=dev), "score": torch.zeros((n, A), dtype=torch.int32, device=dev),
                "insert": KeyInsert(torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.bool, device=dev), None, None),
                "select": Selection(torch.zeros(op["k"], dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))}

    def calls(b, t):
        env.state_key(idx, salt=op["salt"], step_count=op["step_count"], rng=op["rng"], out=b["keys"])
        env.action_mask(idx, out=b["mask"])
        env.agent_distance(idx, types=[op["type"]], through=op["through"], avoid_lava=op["avoid_lava"], out=b["dist"])
        b["score"].copy_(b["dist"])
        t.insert(b["keys"], count=False, out=b["insert"])
        selector.select(b["score"], k=op["k"], out=b["select"])

    def answers(b):
        return {"out.g_keys": b["keys"], "out.g_mask": b["mask"], "out.g_dist": b["dist"], "out.g_is_new": b["insert"].is_new,
                "out.g_index": b["select"].index, "out.g_count": b["select"].count}

    if not is_hip(env):
        b = buffers()
        calls(b, table)
        return answers(b)
    if op["kind"] == "q_graph_again":
        graph, b, _ = ctx["qgraphs"][op["graph"]]
        graph.replay()
        return answers(b)
    # everything bound and allocated before the capture, by one eager pass -- into a table of its own: the insert is no query
    if ctx.get("warm_table") is None:
        ctx["warm_table"] = env.key_table(64)
    ctx["warm_table"].clear()
    b = buffers()
    cur, side, graph = torch.cuda.current_stream(dev), torch.cuda.Stream(dev), torch.cuda.CUDAGraph()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        calls(buffers(), ctx["warm_table"])
        with torch.cuda.graph(graph, stream=side):
            calls(b, table)
    cur.wait_stream(side)
    graph.replay()
    ctx["qgraphs"][op["graph"]] = (graph, b, idx)
    return answers(b)


# ---- looking at an env --------------------------------------------------------------------------------------------------------------

def invariants(env, ctx=""):
    """The layout marker's two rules (include/mgx.h: mgx_step_tracked; BatchedMultiGridEnv._disarm):
    marker[b] >= 0 implies cells[b] == pool[marker[b]] -- `holds` of tests/test_grid_layout_marker.py -- and, on the host's side,
    not armed implies every marker is -1 (what lets _disarm() skip its fill)."""
    root = env._mark["root"]
    loose = int((root != -1).sum())
    assert env._mark["armed"] or loose == 0, \
        f"{ctx}: the marker is not armed, yet {loose} env(s) carry a marker; first env {int((root != -1).nonzero()[0])}"
    m = env._marker.long()
    pool = getattr(env, "_pool", None)
    if pool is None or getattr(env, "_gen", None) is not None:
        assert bool((m == -1).all()), f"{ctx}: an env without a layout pool carries a marker"
        return
    assert bool((m < pool[0].shape[0]).all()), f"{ctx}: a marker names a layout beyond the pool"
    same = (env._cells == pool[0][m.clamp(min=0)]).flatten(1).all(dim=1)
    bad = (m >= 0) & ~same
    n_bad = int(bad.sum())
    assert n_bad == 0, f"{ctx}: env {int(bad.nonzero()[0])} is marked {int(m[bad][0])} but differs from that layout ({n_bad} such env(s))"


def host_state(env, ctx, outs=None, to_host=True) -> dict:
    """Everything `compare` looks at, as host arrays: ONE pass of device-to-host copies per call (to_host=False: the tensors where
    they are, for two envs on one device)."""
    h = (lambda t: t.detach().cpu().numpy()) if to_host else (lambda t: t)
    d = {k: h(getattr(env, k)) for k in STATE + OUTPUTS}
    if env.spec.env_kind != "empty":
        d["aux"] = h(env.aux)
    if getattr(env, "episode", None) is not None:
        d["episode"], d["was_reset"] = h(env.episode), h(env.was_reset)
    if getattr(env, "_gen", None) is not None:
        d["gen_state"] = h(env._gen["gen_state"])
    for n in ("_one_hot", "_full"):
        if getattr(env, n, None) is not None:
            d[n] = h(getattr(env, n))
    if env._stats is not None:
        d.update({"stats." + n: h(t) for n, t in env._stats.tensors.items()})
    for slot, snap in sorted(ctx["snaps"].items()):
        d.update({f"snapshot[{slot}].{m}": h(t) for m, t in snap.tensors.items() if m != "marker"})
    if ctx.get("tm") is not None:
        d.update({f"snapshot[tm].{m}": h(t) for m, t in ctx["tm"].tensors.items() if m != "marker"})
    for k, t in (outs or {}).items():
        if k.startswith("out."):
            d[k] = h(t)
    return d


def first_difference(x, y, batch_axis=0):
    if x.shape != y.shape or x.dtype != y.dtype:
        return f"{x.dtype}{list(x.shape)} against {y.dtype}{list(y.shape)}"
    x, y = np.atleast_1d(x), np.atleast_1d(y)
    bits = {"f": {8: np.uint64, 4: np.uint32}}.get(x.dtype.kind, {}).get(x.dtype.itemsize)
    ne = (np.ascontiguousarray(x).view(bits) != np.ascontiguousarray(y).view(bits)) if bits else (x != y)
    where = np.argwhere(ne)
    if not len(where):
        return "equal"
    idx = tuple(int(v) for v in where[0])
    envs = np.unique(where[:, batch_axis]) if x.ndim > batch_axis else np.zeros(0, int)
    return f"first differing env {int(envs[0]) if len(envs) else '-'} ({len(envs)} env(s) differ), at index {idx}: " \
           f"{x[idx]!r} against {y[idx]!r}"


def assert_same_state(da, db, where, only=None):
    assert set(da) == set(db), f"{where}: the members differ: {sorted(set(da) ^ set(db))}"
    for k in da:
        if only is not None and not only(k):
            continue
        if torch.is_tensor(da[k]):
            if da[k].shape == db[k].shape and torch.equal(da[k], db[k]):
                continue
            da[k], db[k] = da[k].cpu().numpy(), db[k].cpu().numpy()
        if da[k].shape != db[k].shape or da[k].tobytes() != db[k].tobytes():
            raise AssertionError(f"{where}: member {k}: {first_difference(da[k], db[k], 1 if k.startswith('out.') else 0)}")


def where_text(form, B, seed, i, ops) -> str:
    return f"form {form} B={B} seed {seed}: call {i} of {len(ops)}: {describe(ops[i])}"


def check_shadow(env, where):
    """EpisodeStats against the launcher's own accounting (an oracle-backed env)"""
    be = env.backend
    if not isinstance(be, SeqOracle):
        return
    assert (be.shadow is None) == (env._stats is None), where
    if be.shadow is not None:
        for n, t in env._stats.tensors.items():
            if t.numpy().tobytes() != be.shadow[n].tobytes():
                raise AssertionError(f"{where}: the accounting's {n} is not what the launches' outputs make it: "
                                     f"{first_difference(t.numpy(), be.shadow[n])}")


def compare(a, b, ctx_a, ctx_b, where, outs_a=None, outs_b=None, to_host=True):
    """Two envs that took the same calls hold the same bytes -- the state, the engine state beside it, the outputs, what the last call
    handed back, the accounting, the kept snapshots -- and neither has an error to report."""
    da, db = host_state(a, ctx_a, outs_a, to_host), host_state(b, ctx_b, outs_b, to_host)
    assert_same_state(da, db, where)
    a.check_errors(); b.check_errors()
    return da, db


# ---- the census ---------------------------------------------------------------------------------------------------------------------

def census_of(ops_lists, oracles) -> dict:
    """kind -> how often it ran over the lists, and the launchers' own counts"""
    c = {}
    for ops in ops_lists:
        for op in ops:
            c[op["kind"]] = c.get(op["kind"], 0) + 1
            if op["kind"] == "restore" and op["repeated"]:
                c["restore_with_repeated_rows"] = c.get("restore_with_repeated_rows", 0) + 1
        for j, op in enumerate(ops):                          # (the query layer's conditions that a list shows by itself)
            for flag, what in (("hits_touched", "row_query_of_an_env_restored_reset_or_edited_since_the_last"),
                               ("stale", "snapshot_query_older_than_a_pool_or_state_change"),
                               ("first_consumer", "query_as_first_consumer_of_the_chains")):
                if op.get(flag):
                    c[what] = c.get(what, 0) + 1
        seq = [op["value"] is not None for op in ops if op["kind"] == "track"]
        runs = [v for j, v in enumerate(seq) if j == 0 or v != seq[j - 1]]
        if runs[:3] == [True, False, True] or runs[:4] == [False, True, False, True]:
            c["tracking_on_off_on"] = c.get("tracking_on_off_on", 0) + 1
    for be in oracles:
        for k, v in be.census.items():
            c[k] = c.get(k, 0) + v
    return c


_AUX = ["aux_changed_by_a_step", "restore_wrote_a_different_aux", "fork_copied_a_different_aux",
        "stepped_with_hook_order_while_tracking_episodes"]
#: what a hook form's seeds must have met, beside what every form must (conditions on the lists and pools: the oracle alone meets
#: them).  Not asked, because the form cannot reach it:
#:   playground_between   nothing of this: its kind is hook-free, it has no aux and its calls carry no visiting order
#:   rules_pool           the visiting-order items: the declared rules are evaluated per agent, and its calls carry no order;
#:                        its `aux` is the rule table, which no step rewrites: two envs differ in it by their layouts (the twin)
#:   the generator forms  hook_order_changed_the_outcome (the default failure mode and a joint reward are symmetric in the order
#:                        but for RedBlueDoors' first failing toggler, which two agents in a 2 x 4 room seldom reach together),
#:                        and the marker item: a generator env is never armed
HOOK_NEED = {
    "rbd_candidates": _AUX + ["adoption_of_a_slot_with_aux", "hook_success", "hook_failure"],
    # (a generated LockedHallway of this size has the geometric aux -- the same bytes in every env -- until a door is unlocked, which
    # takes a key fetched and carried to its door: more than the 8 steps of an episode.  No step of a random walk rewrites it, and
    # no copy writes another: measured on the oracle, 0 of 4 lists.  LockedHallway's hook state is lh_pool's to show.)
    "lh_candidates": ["adoption_of_a_slot_with_aux", "stepped_with_hook_order_while_tracking_episodes"],
    "rbd_pool": _AUX + ["hook_success", "hook_failure", "hook_order_changed_the_outcome", "stepped_with_hook_order_while_armed"],
    "lh_pool": _AUX + ["hook_order_changed_the_outcome", "stepped_with_hook_order_while_armed"],
    "lh12_pool": _AUX + ["hook_order_changed_the_outcome", "stepped_with_hook_order_while_armed"],
    "rules_pool": ["restore_wrote_a_different_aux", "fork_copied_a_different_aux", "rule_carries_fired", "rule_toggles_at_fired"],
}
#: the same for the query layer.  state_keys_differ_by_hook_state_only needs two rows equal in cells and agents: the pool forms have
#: the twin; a generated env changes its aux only together with its cells (not asked of the generator forms).  A stale door in front
#: of a live agent: RedBlueDoors only
HOOK_QUERY_NEED = {
    "rbd_candidates": ["mask_of_a_stale_door"],
    "rbd_pool": ["state_keys_differ_by_hook_state_only", "mask_of_a_stale_door"],
    "lh_pool": ["state_keys_differ_by_hook_state_only", "distance_over_a_grid_with_an_open_door"],
    "lh12_pool": ["state_keys_differ_by_hook_state_only", "distance_over_a_grid_with_an_open_door"],
    "rules_pool": ["state_keys_differ_by_hook_state_only"],
}


def assert_census(c, form, B, gpu=False, queries=False):
    """Every legal kind at least three times (a GPU-only kind: at least once); the restarts, restores and switches that the
    cross-feature rules are about at least once; for a hook form, HOOK_NEED (and with queries HOOK_QUERY_NEED).  queries: the same for the query kinds, and what the query layer is there to meet
    -- a row query of an env just restored, reset or edited; a snapshot queried after the pool or the state changed under it; an
    insert of new and known keys, a lookup that misses; a selection cut inside a tie and one padded; distances with and without a
    way in one answer; a mask with a clear and a set bit beyond the turns; with the chains, two queries that are their first
    consumer."""
    for k in legal_kinds(form, B, gpu):
        need = 1 if k in GPU_KINDS else 3
        assert c.get(k, 0) >= need, f"form {form}: call kind {k} ran {c.get(k, 0)} time(s), {need} needed: {c}"
    need = ["restore_with_repeated_rows", "tracking_on_off_on", "restored_row_without_the_running_episode"]
    if form not in PLAIN_FORMS:                               # (no restart source: a finished env stays finished)
        need += ["restart_by_truncation", "restored_env_crossed_an_episode_end"]
        # (the box behind the locked door: no random walk of 8 steps picks it up; nor does one unlock every door of a generated
        # LockedHallway, or find a goal on a Playground, which has none: measured on the oracle, 390 of 390 restarts truncations)
        if form not in ("bup_candidates", "lh_candidates", "playground_between"):
            need.append("restart_by_termination")
    need += HOOK_NEED.get(form, [])
    for k in need:
        assert c.get(k, 0) >= 1, f"form {form}: {k} never happened: {c}"
    if not queries:
        return
    for k in legal_query_kinds(form, B, gpu):
        need_k = 1 if k in GPU_QUERY_KINDS else 3
        assert c.get(k, 0) >= need_k, f"form {form}: query kind {k} ran {c.get(k, 0)} time(s), {need_k} needed: {c}"
    need = {"row_query_of_an_env_restored_reset_or_edited_since_the_last": 1, "snapshot_query_older_than_a_pool_or_state_change": 1,
            "insert_of_new_and_known_keys": 1, "lookup_with_a_miss": 1, "select_cut_inside_a_tie": 1, "select_padded": 1,
            "agent_distance_with_and_without_a_way": 1, "mask_with_a_clear_and_a_set_bit_beyond_the_turns": 1}
    need.update({k: 1 for k in HOOK_QUERY_NEED.get(form, [])})
    if gpu and B >= 128:
        need["query_as_first_consumer_of_the_chains"] = 2
    for k, n in need.items():
        assert c.get(k, 0) >= n, f"form {form}: {k} happened {c.get(k, 0)} time(s), {n} needed: {c}"


# ---- pinned cases: the cross-feature rules, one short list each, in the grammar of make_ops ------------------------------------------

def _acts(form, B, seed, *lead):
    r = np.random.default_rng([seed, 99])
    a = r.integers(0, 7, size=lead + (B, SPECS[form].num_agents)).astype(np.int8)
    a[r.random(a.shape) < 0.25] = 2
    return a


def _step(form, B, seed, auto_reset=True, kind="step"):
    return {"kind": kind, "acts": _acts(form, B, seed), "auto_reset": auto_reset}


def _restore(slot, env_ids, rows=None, carries=False):
    e = None if env_ids is None else np.asarray(env_ids, np.int64)
    rows = None if rows is None else np.asarray(rows, np.int64)
    return {"kind": "restore", "slot": slot, "env_ids": e, "rows": rows, "check": False,
            "repeated": rows is not None and len(np.unique(rows)) < len(rows), "carries": carries}


def _edit(form, env_ids, y, x, triple=(9, 0, 0)):
    t = np.asarray(triple, np.uint8)
    return {"kind": "edit", "env_ids": np.asarray(env_ids, np.int64), "y": y, "x": x,
            "value": int(layouts.pack_cells_for(SPECS[form], t[None])[0]), "triple": t}


def _snapshot(slot, env_ids=None):
    return {"kind": "snapshot", "slot": slot, "env_ids": None if env_ids is None else np.asarray(env_ids, np.int64)}


def pinned_edit_then_step():
    """a cell edit through `cells`, then step(auto_reset): the step sees the edit (the marker's promise was taken back)"""
    form, B = "pool1", 130
    ids = [0, 1, 17, 64, 129]

    def unmarked(env, where):
        assert bool((env._marker[ids] == -1).all()), where
    ops = [_step(form, B, 1), _step(form, B, 2), {"kind": "reset", "seed": None, "mask": np.arange(B) % 2 == 0},
           _edit(form, ids, 3, 3), _step(form, B, 3), {"kind": "gen_obs", "one_hot": False}, _step(form, B, 4)]
    return {"form": form, "B": B, "ops": ops, "checks": {3: unmarked}}


def pinned_armed_snapshot_after_cells():
    """a snapshot taken while the marker was armed, restored after `cells` disarmed the env: the restored rows are marked again,
    and they ARE their layout again"""
    form, B = "pool1", 130
    ids = np.arange(0, B, 3)

    def armed(env, where):
        assert env._mark["armed"] and bool((env._marker == 0).all()), where

    def disarmed(env, where):
        assert not env._mark["armed"] and bool((env._marker == -1).all()), where

    def rearmed(env, where):
        want = torch.full((B,), -1, dtype=torch.int32)
        want[torch.from_numpy(ids)] = 0
        assert env._mark["armed"] and torch.equal(env._marker.cpu(), want), where
    ops = [{"kind": "reset", "seed": 5, "mask": None}, _snapshot(0), _edit(form, [0, 3, 4, 129], 1, 2), _restore(0, ids, ids),
           _step(form, B, 1), _step(form, B, 2), _step(form, B, 3, auto_reset=False), _step(form, B, 4)]
    return {"form": form, "B": B, "ops": ops, "checks": {1: armed, 2: disarmed, 3: rearmed}}


def pinned_restore_after_refill():
    """a snapshot restored after an in-place refill of the pool: its layout indices name other layouts now -- the markers of the
    restored rows come out -1"""
    form, B = "pool1", 130
    ids = np.array([2, 64, 65, 100])
    g, a, x = small_pool(SPECS[form], 1, np.random.default_rng(8))

    def unknown(env, where):
        m = env._marker.cpu()
        assert bool((m[torch.from_numpy(ids)] == -1).all()) and int((m == 0).sum()) == 0, where
    ops = [{"kind": "reset", "seed": None, "mask": None}, _snapshot(0), {"kind": "pool_refill", "grids": g, "agents": a, "aux": x},
           _restore(0, ids, ids), _step(form, B, 1), _step(form, B, 2)]
    return {"form": form, "B": B, "ops": ops, "checks": {3: unknown}}


def pinned_restore_before_an_adoption():
    """restore / reset(mask) / seed between a staged generator's snapshot of np_random (`lead` = 4 steps before the truncation at 6)
    and the truncation that would adopt the slot made from it: the slots are a cache"""
    form, B = "gen_between", 130
    ops = [_step(form, B, 1), _step(form, B, 2), _snapshot(0), _step(form, B, 3), _step(form, B, 4),
           _restore(0, np.arange(0, B, 2), np.arange(0, B, 2)), {"kind": "seed", "seed": 9},
           {"kind": "reset", "seed": None, "mask": (np.arange(B) % 5 == 0).astype(np.uint8)}]
    ops += [_step(form, B, 5 + t) for t in range(7)]
    return {"form": form, "B": B, "ops": ops}


def pinned_restore_before_an_adoption_candidates():
    """the same with candidates: every episode end an adoption"""
    case = pinned_restore_before_an_adoption()
    return dict(case, form="gen_candidates")


def pinned_track_between_hot_path_steps():
    """track_episodes() between two steps of the hot-path entry: the entry bound before the switch steps without (or with) the
    accounting, and must not be the one that runs after it"""
    form, B = "pool1", 130
    ops = [_step(form, B, 1), _step(form, B, 2), {"kind": "track", "value": False}, _step(form, B, 3), _step(form, B, 4),
           {"kind": "track", "value": None}, _step(form, B, 5), {"kind": "track", "value": True}, _step(form, B, 6),
           {"kind": "rollout", "acts": _acts(form, B, 7, 3), "auto_reset": True}, _step(form, B, 8, auto_reset=False),
           {"kind": "reset", "seed": None, "mask": np.arange(B) % 3 == 0}, _step(form, B, 9)]
    return {"form": form, "B": B, "ops": ops}


def pinned_load_state_dict_stages_the_generator():
    """load_state_dict of an unstaged generator env makes it a staged one; a restore of an older snapshot follows"""
    form, B = "gen", 130

    def staged(env, where):
        assert env._gen.get("stage") is not None, where
    ids = np.arange(1, B, 2)
    ops = [_step(form, B, 1), _step(form, B, 2), _snapshot(0), _step(form, B, 3), _step(form, B, 4), _step(form, B, 5),
           {"kind": "load_state_dict"}, _step(form, B, 6), _step(form, B, 7), _restore(0, ids, ids)]
    ops += [_step(form, B, 8 + t) for t in range(7)]
    return {"form": form, "B": B, "ops": ops, "checks": {6: staged}}


def pinned_generated_rollout_of_unaligned_steps():
    """rollout(auto_reset=True) with a layout generator is T launches of the one-step kernel over the [t] slices of its outputs: at
    130 envs x 2 agents x 27 bytes a step's observations are no multiple of 16 bytes, and slice 1 is not aligned as that kernel asks
    (found by the random sequences: the launcher refused it with step 0 already taken)"""
    form, B = "gen_between", 130
    assert (B * SPECS[form].num_agents * 27) % 16
    ops = [_step(form, B, 1), {"kind": "rollout", "acts": _acts(form, B, 2, 4), "auto_reset": True}, _step(form, B, 3),
           {"kind": "rollout", "acts": _acts(form, B, 4, 3), "auto_reset": True}, {"kind": "track", "value": True},
           {"kind": "rollout", "acts": _acts(form, B, 5, 4), "auto_reset": True}, _step(form, B, 6)]
    return {"form": form, "B": B, "ops": ops}


def _order(B, A, seed, *lead):
    return np.argsort(np.random.default_rng([seed, 98]).random(lead + (B, A)), axis=-1).astype(np.uint8)


def _toggles(form, B, seed, auto_reset=False, order=True, p=0.8):
    """a step in which most agents toggle what they face (the hook pools' starts face their doors), in a visiting order"""
    a = _acts(form, B, seed)
    a[np.random.default_rng([seed, 97]).random(a.shape) < p] = hs.TOGGLE
    return {"kind": "step", "acts": a, "auto_reset": auto_reset, "hook_order": _order(B, a.shape[1], seed) if order else None}


def pinned_restore_of_a_changed_aux():
    """RedBlueDoors: a snapshot of fresh starts, a step of toggles that rewrites aux (the failed openings raise the stale flag, the
    toggles at a stale door lower it), a restore of every other env, and the same toggles again: what they do depends on the flag --
    a restore that left aux as it was would show in that step"""
    form, B = "rbd_pool", 130
    ids = np.arange(0, B, 2)
    kept = {}

    def rewritten(env, where):
        kept["aux"] = env.aux.cpu().clone()
        assert int((kept["aux"][:, 4] != kept["start"][:, 4]).sum()) >= 8, f"{where}: the step did not rewrite the stale flags"

    def start(env, where):
        kept["start"] = env.aux.cpu().clone()

    def restored(env, where):
        aux, t = env.aux.cpu(), torch.from_numpy(ids)
        assert torch.equal(aux[t], kept["start"][t]) and not torch.equal(aux[t], kept["aux"][t]), f"{where}: aux of the restored envs"
        others = torch.from_numpy(np.arange(1, B, 2))
        assert torch.equal(aux[others], kept["aux"][others]), f"{where}: aux of the other envs"
    ops = [{"kind": "reset", "seed": 5, "mask": None}, _snapshot(0), _toggles(form, B, 1), _restore(0, ids, ids), _toggles(form, B, 1),
           _toggles(form, B, 2, auto_reset=True), _toggles(form, B, 3, auto_reset=True, order=False)]
    return {"form": form, "B": B, "ops": ops, "checks": {1: start, 2: rewritten, 3: restored}}


def pinned_reset_between_launch_and_adoption():
    """LockedHallway with one candidate per env: reset(seed, mask) between the generator launch that made the candidates (every
    lead / 2 = 2 steps) and the truncation at 8 that would adopt them -- the chosen envs' episode counters moved on, their slots are
    stale, and the adoption must not take them; the steps come with and without a visiting order"""
    form, B = "lh_candidates", 130

    def launched(env, where):
        if is_hip(env):                                       # (the oracle generates in place: it keeps no slots)
            assert bool((env._gen["stage"]["tag"] != -1).any()), f"{where}: no candidate has been made yet"
    ops = [_toggles(form, B, 1, auto_reset=True, p=0.2), _step(form, B, 2), _toggles(form, B, 3, auto_reset=True, p=0.2), _step(form, B, 4),
           {"kind": "reset", "seed": 9, "mask": (np.arange(B) % 3 == 0).astype(np.uint8)}, _step(form, B, 5),
           {"kind": "reset", "seed": None, "mask": np.arange(B) % 5 == 0}]
    ops += [_toggles(form, B, 6 + t, auto_reset=True, order=bool(t % 2), p=0.2) for t in range(9)]
    return {"form": form, "B": B, "ops": ops, "checks": {3: launched}}


def pinned_hook_order_after_hot_path_steps():
    """step(hook_order=...) directly behind steps of the bound hot-path entry on an armed pool: the visiting order sends the call
    through the slow entry, which must keep (auto_reset: the tracked step) or take back (no auto_reset) the marker's promise itself"""
    form, B = "rbd_pool", 130

    def armed(env, where):
        if is_hip(env):                                       # (an oracle-backed env has no tracked step: only a one-layout pool arms it)
            assert env._mark["armed"] and env._bound.get((True, False), (0, 0, False))[2], f"{where}: not armed by a tracked hot-path step"

    def disarmed(env, where):
        assert not env._mark["armed"] and bool((env._marker == -1).all()), where
    ops = [_toggles(form, B, 1, auto_reset=True, order=False), _toggles(form, B, 2, auto_reset=True, order=False),
           _toggles(form, B, 3, auto_reset=True, order=False), _toggles(form, B, 4, auto_reset=True), _toggles(form, B, 5, auto_reset=True, order=False),
           _toggles(form, B, 6, auto_reset=True), _toggles(form, B, 7), _toggles(form, B, 8, auto_reset=True, order=False),
           _toggles(form, B, 9, auto_reset=True)]
    return {"form": form, "B": B, "ops": ops, "checks": {2: armed, 3: armed, 4: armed, 6: disarmed}}


def pinned_load_state_dict_of_a_hook_pool():
    """load_state_dict of a hook pool form -- the pool's aux travels in the dict --, then auto-reset steps: the envs that restart
    take their layout's aux -- the door positions and the stale flag -- with its cells"""
    form, B = "rbd_pool", 130
    kept = {}

    def before(env, where):
        kept["pool_aux"], kept["aux"] = env._pool[2].cpu().clone(), env.aux.cpu().clone()
        assert bool(kept["pool_aux"].any()) and len({bytes(r) for r in kept["pool_aux"].numpy()}) > 1, where

    def restarted(env, where):
        assert int(env.was_reset.sum()) > 0, f"{where}: no env restarted from the loaded pool"

    def loaded(env, where):
        assert env._pool[2] is not None and torch.equal(env._pool[2].cpu(), kept["pool_aux"]), f"{where}: the pool's aux"
        assert torch.equal(env.aux.cpu(), kept["aux"]), f"{where}: the envs' aux"
    ops = [_toggles(form, B, 1), _toggles(form, B, 2), {"kind": "load_state_dict"}, _toggles(form, B, 3, auto_reset=True),
           _toggles(form, B, 4, auto_reset=True, order=False), _toggles(form, B, 5, auto_reset=True), _toggles(form, B, 6, auto_reset=True)]
    return {"form": form, "B": B, "ops": ops, "checks": {1: before, 2: loaded, 3: restarted}}


PINNED = {"edit_then_step": pinned_edit_then_step, "generated_rollout_of_unaligned_steps": pinned_generated_rollout_of_unaligned_steps, "armed_snapshot_after_cells": pinned_armed_snapshot_after_cells,
          "restore_after_refill": pinned_restore_after_refill, "restore_before_an_adoption": pinned_restore_before_an_adoption,
          "restore_before_an_adoption_candidates": pinned_restore_before_an_adoption_candidates,
          "track_between_hot_path_steps": pinned_track_between_hot_path_steps,
          "load_state_dict_stages_the_generator": pinned_load_state_dict_stages_the_generator,
          "restore_of_a_changed_aux": pinned_restore_of_a_changed_aux,
          "reset_between_launch_and_adoption": pinned_reset_between_launch_and_adoption,
          "hook_order_after_hot_path_steps": pinned_hook_order_after_hot_path_steps,
          "load_state_dict_of_a_hook_pool": pinned_load_state_dict_of_a_hook_pool}
