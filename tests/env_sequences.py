"""Random call sequences through BatchedMultiGridEnv: the driver of tests/test_env_sequences.py (two oracle-backed envs, no GPU) and
tests/test_env_sequences_gpu.py (HIP against the oracle).  No tests in here.

  * `make_ops(form, B, n_ops, seed)` lists every call up front, arguments included (NumPy values).  Whether a call is legal is decided
    from host-known facts alone -- the form, whether the accounting is on, B >= 128, which snapshots and graphs are kept and what
    they carry -- never from a result: two envs given one list do the same thing, and (form, B, n_ops, seed) names a failure.
  * `apply(env, op, ctx)` performs one call on either kind of env (the GPU-only kinds have an eager equivalent on the oracle).
  * `compare(a, b, ...)` holds two envs to each other byte for byte; `invariants(env)` are the layout marker's two rules;
    `SeqOracle` is the CPU model of every launcher -- CopyOracle(StatsOracle(SelectOracle(OracleBackend))) -- with a one-hot gen_obs,
    an accounting of its own fed from what the launches hand back (`shadow`: what EpisodeStats must hold whatever the host logic
    called), and the census of what a run went through."""
import weakref

import numpy as np
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib, layouts
from oracle import binding as ob
from tests import util
from tests.test_env_snapshot import TRIO, CopyOracle
from tests.test_episode_stats import model_restart, model_stats, new_state

NONE, BEFORE, AFTER = _lib.RESTART_NONE, _lib.RESTART_BEFORE, _lib.RESTART_AFTER
STATE = ("_cells", "agents", "rng", "step_count")
OUTPUTS = ("obs", "dir", "reward", "terminated", "truncated")
FORMS = ("plain", "pool1", "pool4_objects", "pool_compact", "gen", "gen_candidates", "gen_between", "bup_candidates")
#: the batch whose launches READ the layout marker (more than 2048 wavefronts, one layout): tests/test_env_sequences_gpu.py
BIG_FORMS = ("big_empty1", "big_objects1")
#: `plain` and `pool1` on shapes of their own -- grids that are not square --, which the HIP env steps on a kernel compiled at run time
#: (make_env(specialise=True); a registration serves every env of its geometry for the rest of the process: no other form, and no
#: other test file, uses these shapes): tests/test_jit_forms_gpu.py
JIT_FORMS = ("plain_jit", "pool1_jit")
PLAIN_FORMS = ("plain", "plain_jit")                         # no restart source: load_state alone
POOL1_FORMS = ("pool1", "pool1_jit")
POOL_FORMS = ("pool1", "pool4_objects", "pool_compact") + BIG_FORMS + ("pool1_jit",)
GEN_FORMS = ("gen", "gen_candidates", "gen_between", "bup_candidates")
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
}
FIRST_ENV = {"pool4_objects": 11, "gen_between": 11, "bup_candidates": 11}
#: the pool sizes a form alternates between when `pool_replace` gives it another K
POOL_K = {"pool1": (1, 2), "pool4_objects": (4, 3), "pool_compact": (2, 3), "big_empty1": (1, 2), "big_objects1": (1, 2),
          "pool1_jit": (1, 2)}
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
              "gen_obs", "full_obs", "capture_replay", "step_chains")
#: relative frequencies; every legal kind must run at least three times over a form's seeds (the census of the tests)
WEIGHTS = {"step": 8, "step_one_hot": 2, "rollout": 3, "reset_done": 2, "reset": 3, "snapshot": 4, "snapshot_out": 2, "restore": 5,
           "fork": 2, "edit": 3, "load_state_dict": 1.6, "pool_refill": 1.6, "pool_replace": 1.4, "track": 3.0, "reset_totals": 2.6,
           "stats_lsd": 2.6, "seed": 2, "gen_obs": 2, "full_obs": 2, "one_hot_obs": 2, "split": 2, "capture_replay": 2.5,
           "graph_again": 4, "persistent": 3, "step_chains": 4}


# ---- the oracle launcher ------------------------------------------------------------------------------------------------------------

class SeqOracle(CopyOracle):
    """The CPU model of every launcher, and what watches a run:

    shadow   the accounting's tensors as they must be, or None while it is off: updated HERE from what each stepping / restart launch
             hands back, by the sequential model -- not by the accounting calls the host logic makes, which it checks.  A restore
             takes the running trio of the rows it wrote from the env (the env copy is held to its own model elsewhere).
    census   what happened: restarts by truncation / termination, a restored env that crossed an episode end, ...
    Sub-shards of split() share the launcher: their rows are found by the storage offset of their `step_count` view."""

    def __init__(self, spec):
        super().__init__(spec)
        self.shadow, self.census, self.env = None, {}, None
        self._nested, self._faking = 0, False
        self.restored = None

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
        self._nested += 1
        try:
            super().step(B, grid, agents, rng, step_count, actions, target, err, obs, dirs, reward, terminated, truncated, **kw)
        finally:
            self._nested -= 1
        if self.shadow is not None and self._nested == 0:
            ar = kw.get("auto_reset")
            model_stats(self._shadow_rows(self._rows(step_count, B)), reward.numpy(), terminated.numpy(), truncated.numpy(),
                        ar[3].numpy() if ar is not None else None, BEFORE if ar is not None else NONE)

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
        self._restarted(rows, step_count, B, was_reset)

    def _as_done(self, sel, agents, step_count, call):
        self._faking = True
        try:
            super()._as_done(sel, agents, step_count, call)
        finally:
            self._faking = False

    def env_copy(self, n, src, src_rows, src_idx, dst, dst_rows, dst_idx, stage_tag, stage_mode, marker_fill, bad):
        super().env_copy(n, src, src_rows, src_idx, dst, dst_rows, dst_idx, stage_tag, stage_mode, marker_fill, bad)
        env = self.env() if self.env is not None else None
        if env is None or dst["cells"].data_ptr() != env._cells.data_ptr():
            return                                         # (a snapshot: the env is the source)
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


def pool_content(form, K, r):
    """the pool a `pool_refill` / `pool_replace` installs"""
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


def make_ops(form, B, n_ops, seed, gpu=False, stretch=None, weights=None, kinds=None, every_third=None):
    """The whole list of calls of one sequence.

    gpu          the GPU-only kinds are in
    stretch      (s, e): call s is `tm_begin` (a snapshot of the whole batch, the kept ones forgotten), and the calls s+1 .. e-1 are
                 PURE_KINDS that use only snapshots taken after s -- what the time machine records, restores and repeats
    kinds        restrict the kinds drawn (the large-batch test); every_third: that call at every third index instead of a draw"""
    r = np.random.default_rng([seed, B, (FORMS + BIG_FORMS + JIT_FORMS).index(form)])
    spec = SPECS[form]
    A, H, W = spec.num_agents, spec.height, spec.width
    source = form not in PLAIN_FORMS
    w = dict(WEIGHTS, **(weights or {}))
    allowed = set(legal_kinds(form, B, gpu)) if kinds is None else set(kinds)
    S = {"tracking": None, "snaps": {}, "graphs": {}, "version": 0, "persistent": 0, "K": POOL_K.get(form, (0,))[0], "next_slot": 0,
         "next_graph": 0, "staged": form in ("gen_candidates", "gen_between", "bup_candidates")}

    def actions(*lead):
        a = r.integers(0, 7, size=lead + (B, A)).astype(np.int8)
        a[r.random(lead + (B, A)) < 0.25] = 2                 # forward: episodes end by reaching something, too
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
            S["snaps"][slot] = {"rows": B if e is None else len(e), "tracked": tracked, "pure": pure, "all": e is None}
            op.update(slot=slot, env_ids=e)
        elif kind == "snapshot_out":
            fit = [s for s in usable(pure) if S["snaps"][s]["tracked"] == tracked]
            if not fit:
                return None
            slot = int(r.choice(fit))
            v = S["snaps"][slot]
            e = None if v["all"] and r.random() < 0.5 else ids(v["rows"])
            v.update(pure=pure, all=v["all"] and e is None)
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

    ops, ran = [], {}
    for i in range(n_ops):
        pure = stretch is not None and stretch[0] < i < stretch[1]
        if stretch is not None and i == stretch[0]:
            S["snaps"] = {}
            ops.append({"kind": "tm_begin"})
            continue
        if every_third is not None and i % 3 == 2:
            ops.append({"kind": "step", "acts": actions(), "auto_reset": True})
            continue
        if every_third is not None and i % 9 == 3:           # (an edit right behind a step whose restarts marked their envs)
            ops.append(draw("edit", pure))
            continue
        if pure and i == stretch[0] + 3:                     # (so that the stretch has a snapshot of its own to restore and fork from)
            ops.append(draw("snapshot", pure))
            continue
        names = sorted(k for k in allowed if not pure or k in PURE_KINDS)
        # (a kind the list has met less than twice is four times as likely: every list holds every kind its form allows)
        p = np.array([w[k] * (4 if ran.get(k, 0) < 2 else 1) for k in names], float)
        while True:
            op = draw(names[int(r.choice(len(names), p=p / p.sum()))], pure)
            if op is not None:
                break
        ran[op["kind"]] = ran.get(op["kind"], 0) + 1
        ops.append(op)
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
    return {"snaps": {}, "graphs": {}, "tm": None}


def is_hip(env) -> bool:
    return getattr(env.backend, "name", "") == "hip"


def apply(env, op, ctx) -> dict:
    """One call on `env`.  Returns what the call wrote or handed back that is not part of the env state: name -> tensor (the env's
    own output buffers by name, a rollout's dict under 'out.<key>')."""
    dev, kind, hip = env.device, op["kind"], is_hip(env)
    be = env.backend

    def dv(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def outputs(auto_reset=False, one_hot=False):
        names = (("_one_hot",) if one_hot else ("obs",)) + OUTPUTS[1:] + (("was_reset",) if auto_reset else ())
        return {n: getattr(env, n) for n in names}

    def steps(acts, auto_reset, times=1):
        for _ in range(times):
            for t in range(acts.shape[0]):
                env.step(dv(acts[t]), auto_reset=auto_reset)
        return outputs(auto_reset)

    if kind == "step":
        env.step(dv(op["acts"]), auto_reset=op["auto_reset"])
        return outputs(op["auto_reset"])
    if kind == "step_one_hot":
        env.step(dv(op["acts"]), auto_reset=op["auto_reset"], one_hot=True)
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
        env.fork(dv(op["src"]), dv(op["dst"]), check=op["check"])
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
                c.step(dv(op["acts"][t, lo:hi]), auto_reset=op["auto_reset"])
                invariants(c, f"sub-shard [{lo}, {hi}) step {t}")
        return outputs(op["auto_reset"])
    # ---- the GPU-only kinds, and what they are on the oracle
    if kind == "capture_replay":
        if not hip:
            if op["keep"] is not None:
                ctx["graphs"][op["keep"]] = True
            return steps(op["acts"], op["auto_reset"], times=2)
        graph = env.capture_steps(dv(op["acts"]), auto_reset=op["auto_reset"], sub_shards=op["sub_shards"])
        graph.replay(); graph.replay()
        if op["keep"] is not None:
            ctx["graphs"][op["keep"]] = graph
        return outputs(op["auto_reset"])
    if kind == "graph_again":
        if not hip:
            return steps(op["acts"], op["auto_reset"])
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
            return steps(op["acts"][None], op["auto_reset"])
        env.step(dv(op["acts"]), auto_reset=op["auto_reset"], sub_shards=2)
        env.join()
        return outputs(op["auto_reset"])
    raise ValueError(f"unknown call kind {kind!r}")


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
        seq = [op["value"] is not None for op in ops if op["kind"] == "track"]
        runs = [v for j, v in enumerate(seq) if j == 0 or v != seq[j - 1]]
        if runs[:3] == [True, False, True] or runs[:4] == [False, True, False, True]:
            c["tracking_on_off_on"] = c.get("tracking_on_off_on", 0) + 1
    for be in oracles:
        for k, v in be.census.items():
            c[k] = c.get(k, 0) + v
    return c


def assert_census(c, form, B, gpu=False):
    """Every legal kind at least three times (a GPU-only kind: at least once); the restarts, restores and switches that the
    cross-feature rules are about at least once."""
    for k in legal_kinds(form, B, gpu):
        need = 1 if k in GPU_KINDS else 3
        assert c.get(k, 0) >= need, f"form {form}: call kind {k} ran {c.get(k, 0)} time(s), {need} needed: {c}"
    need = ["restore_with_repeated_rows", "tracking_on_off_on", "restored_row_without_the_running_episode"]
    if form not in PLAIN_FORMS:                               # (no restart source: a finished env stays finished)
        need += ["restart_by_truncation", "restored_env_crossed_an_episode_end"]
        if form != "bup_candidates":                          # (the box behind the locked door: no random walk of 8 steps picks it up)
            need.append("restart_by_termination")
    for k in need:
        assert c.get(k, 0) >= 1, f"form {form}: {k} never happened: {c}"


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


PINNED = {"edit_then_step": pinned_edit_then_step, "generated_rollout_of_unaligned_steps": pinned_generated_rollout_of_unaligned_steps, "armed_snapshot_after_cells": pinned_armed_snapshot_after_cells,
          "restore_after_refill": pinned_restore_after_refill, "restore_before_an_adoption": pinned_restore_before_an_adoption,
          "restore_before_an_adoption_candidates": pinned_restore_before_an_adoption_candidates,
          "track_between_hot_path_steps": pinned_track_between_hot_path_steps,
          "load_state_dict_stages_the_generator": pinned_load_state_dict_stages_the_generator}
