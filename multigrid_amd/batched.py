"""BatchedMultiGridEnv: B independent MultiGrid environments resident in HBM, stepped by one fused HIP kernel.

This is the tensor-level form of `multigrid.base.MultiGridEnv` (multigrid/base.py:36-841 of the reference):
`reset` / `step` / `gen_obs` keep the reference's meaning, with dict-of-agents replaced by a leading
(batch, agent) shape.  The per-env dict API lives in multigrid_amd/env.py on top of this class.

State (device tensors, layouts in include/mgx.h):
    cells i16[B,H,W] (packed grid cells, include/mgx.h MgxCell; `grid` = the same as (type, color, state) bytes
    u8[B,H,W,3])   agents u8[B,A,8]   rng i64[B,4] (PCG64 words)   step_count i32[B]   aux u8[B,16]
Outputs of `step` (pre-allocated, overwritten by every call -- clone what you keep):
    obs u8[B,A,v,v,3]  dir u8[B,A]  reward f64[B,A]  terminated u8[B,A]  truncated u8[B]
"""
from __future__ import annotations

import os
import weakref

import numpy as np
import torch

from . import _lib, layouts, rng as rnglib, row_queries
from .constants import NO_ACTION, Action, Type
from .row_queries import RowSet, _key_args, _out
from .spec import EnvSpec

INT32_MAX = 2 ** 31 - 1


class StepGraph:
    """A captured hipGraph of env steps (BatchedMultiGridEnv.capture_steps)."""

    def __init__(self, env, graph, sub_shards, keep):
        self.env, self.graph, self.sub_shards = env, graph, sub_shards
        self._version = env._layout_version
        self._keep = keep                # the sub-shards' pre-bound launchers, their streams, the action tensors

    def replay(self):
        if self.env._layout_version != self._version:
            raise RuntimeError("this graph was captured before set_layout_pool() / set_layout_generator() replaced the layout "
                               "tensors it holds pointers to: capture_steps() again")
        if not getattr(self, "_tracked", False):     # (steps that write cells without keeping the layout marker)
            self.env._disarm()
        self.graph.replay()


class EpisodeStats:
    """Returns, lengths and outcomes of the episodes of a BatchedMultiGridEnv, kept on the device by the env itself
    (`BatchedMultiGridEnv.track_episodes()`; the rule: include/mgx.h "EPISODE ACCOUNTING").  The tensors, read-only by convention:

        cur_return f64[B,A]  cur_length i32[B]   the running episode        over u8[B]  closed, and not restarted since
        last_return f64[B,A] last_length i32[B]  the episode closed last
        sum_return f64[B,A]  sum_length i64[B]   over all closed episodes   counts i32[B,4]  closed, terminated, rewarded, aborted

    Everything is per env: a batch-level figure is a `sum()` at logging time (`summary()`)."""

    TENSORS = (("cur_return", torch.float64, True), ("cur_length", torch.int32, False), ("over", torch.uint8, False),
               ("last_return", torch.float64, True), ("last_length", torch.int32, False), ("sum_return", torch.float64, True),
               ("sum_length", torch.int64, False), ("counts", torch.int32, 4))

    def __init__(self, batch: int, num_agents: int, device, trace: bool = False, _tensors=None):
        self.batch, self.num_agents, self.trace = int(batch), int(num_agents), bool(trace)
        if _tensors is None:
            _tensors = {}
            for name, dt, per in self.TENSORS:
                shape = (self.batch, num_agents) if per is True else ((self.batch, per) if per else (self.batch,))
                _tensors[name] = torch.zeros(shape, dtype=dt, device=device)
        self.tensors = _tensors          # name -> tensor, in the order of struct MgxEpisodeStats
        for name, t in _tensors.items():
            setattr(self, name, t)

    def _slice(self, lo: int, hi: int) -> "EpisodeStats":
        """The envs [lo, hi) as views (a sub-shard's share: BatchedMultiGridEnv.split)."""
        return EpisodeStats(hi - lo, self.num_agents, None, self.trace, {n: t[lo:hi] for n, t in self.tensors.items()})

    def summary(self) -> dict:
        """The closed episodes of the whole batch as Python numbers, after ONE device-to-host copy: episodes, mean_return (per
        agent), mean_length, the shares terminated / rewarded of the closed episodes, and the number aborted."""
        A = self.num_agents
        v = torch.cat((self.counts.sum(dim=0).to(torch.float64), self.sum_length.sum().to(torch.float64).reshape(1),
                       self.sum_return.sum(dim=0))).cpu().tolist()
        n = int(v[0])
        d = float(max(n, 1))
        return {"episodes": n, "mean_return": [x / d for x in v[5:5 + A]], "mean_length": v[4] / d, "terminated": v[1] / d,
                "rewarded": v[2] / d, "aborted": int(v[3])}

    def reset_totals(self):
        """Zero the totals and the counters (a new logging window); running episodes are left alone."""
        self.sum_return.zero_(); self.sum_length.zero_(); self.counts.zero_()

    def state_dict(self) -> dict:
        return {n: t.cpu().clone() for n, t in self.tensors.items()}

    def load_state_dict(self, sd: dict):
        for n, t in self.tensors.items():
            if tuple(sd[n].shape) != tuple(t.shape):
                raise ValueError(f"episode stats: {n} has shape {tuple(sd[n].shape)}, expected {tuple(t.shape)}")
        for n, t in self.tensors.items():
            t.copy_(sd[n])


class EnvSnapshot:
    """The state of `rows` envs of a BatchedMultiGridEnv as a value (`BatchedMultiGridEnv.snapshot()`), in device tensors of its own
    (`.tensors`: member -> tensor with `rows` leading rows, the members of include/mgx.h MgxEnvRows the env carried):

        cells (the env's own format)  agents  rng  step_count  aux  marker
        episode     with a layout pool or a generator        gen_state   with a generator
        cur_return, cur_length, over   the running episode, while track_episodes() was on

    What a step hands back (obs, reward, ...) is no part of it: `gen_obs()` after a restore.  It remembers the spec, the kind of
    restart source, and which env it came from at which `_layout_version` (only there do its layout markers mean anything)."""

    MEMBERS = tuple(n for n, _ in _lib.MgxEnvRows._fields_[:-1])

    def __init__(self, spec, rows: int, tensors: dict, source: tuple):
        self.spec, self.rows, self.tensors, self.source = spec, int(rows), tensors, source
        self.layout_version, self._layout_epoch, self._env, self._armed, self._seeded = 0, 0, None, False, False

    def _taken_from(self, env):
        self.layout_version, self._layout_epoch, self._env = env._layout_version, env._layout_epoch, weakref.ref(env)
        self._armed, self._seeded = bool(env._mark["armed"]), env._seeded

    def _is_of(self, env) -> bool:
        """Taken from this very env, and its layout pool has not been replaced or refilled since."""
        return (self._env is not None and self._env() is env and self.layout_version == env._layout_version
                and self._layout_epoch == env._layout_epoch)

    @property
    def device(self):
        return self.tensors["cells"].device

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors.values())

    def _row_set(self, what: str) -> RowSet:
        """This snapshot's own tensors as the rows of a query (row_queries.py), launched by the env that took it."""
        env = self._env() if self._env is not None else None
        if env is None:
            raise RuntimeError(f"{what}: the env this snapshot was taken from is gone (its backend makes the launch)")
        env.join()
        return RowSet(what, env, self.tensors, self.rows, self.device, "rows")

    def state_key(self, rows: torch.Tensor | None = None, *, salt: int = 0, step_count: bool = False, rng: bool = False,
                  out: torch.Tensor | None = None) -> torch.Tensor:
        """The keys of the snapshot rows `rows` (contiguous int64 [n] on the snapshot's device; None = every row, in order) -- the
        launch of `BatchedMultiGridEnv.state_key()` over the snapshot's own tensors, through the backend of the env that took it: a
        row's key is the key that env had when the snapshot was taken.  A row outside [0, rows) leaves its key as it was and is
        reported by that env's `check_errors()`."""
        return row_queries.state_key(self._row_set("state_key"), rows, salt, step_count, rng, out)

    def action_mask(self, rows: torch.Tensor | None = None, *, expand: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
        """The effective-action masks of the snapshot rows `rows` (contiguous int64 [n] on the snapshot's device; None = every row, in
        order) -- the launch of `BatchedMultiGridEnv.action_mask()` over the snapshot's own tensors, through the backend of the env
        that took it: a row's masks are the masks that env had when the snapshot was taken.  A row outside [0, rows) leaves its masks
        as they were and is reported by that env's `check_errors()`."""
        return row_queries.action_mask(self._row_set("action_mask"), rows, expand, out)

    def distance_field(self, rows: torch.Tensor | None = None, *, types=None, colors=None, agents=None, points=None, through=(),
                       avoid_lava: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
        """The walking-distance fields of the snapshot rows `rows` (contiguous int64 [n] on the snapshot's device; None = every row,
        in order) -- the launch of `BatchedMultiGridEnv.distance_field()` over the snapshot's own tensors, through the backend of the
        env that took it.  A row outside [0, rows) leaves its field as it was and is reported by that env's `check_errors()`."""
        query = dict(types=types, colors=colors, agents=agents, points=points, through=through, avoid_lava=avoid_lava)
        return row_queries.distance(self._row_set("distance_field"), rows, query, out, True)

    def agent_distance(self, rows: torch.Tensor | None = None, *, types=None, colors=None, agents=None, points=None, through=(),
                       avoid_lava: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
        """The agents' walking distances in the snapshot rows `rows`: `BatchedMultiGridEnv.agent_distance()` over the snapshot's
        own tensors (see `distance_field()` above)."""
        query = dict(types=types, colors=colors, agents=agents, points=points, through=through, avoid_lava=avoid_lava)
        return row_queries.distance(self._row_set("agent_distance"), rows, query, out, False)


class PersistentSession:
    """Closed-loop stepping without a kernel boundary per step (include/mgx.h: mgx_step_persistent): ONE launch of the step kernel
    stays resident on a stream of its own, keeps the env state in LDS, takes each step's actions as tagged granules and publishes
    a per-wavefront flag behind the step's outputs.  For batches in the latency regime (C2, C4's 8-GPU share, C3), where the launch
    boundary and the state reload are a third of a step.  Made by `BatchedMultiGridEnv.persistent()`; use as a context manager.

        obs, dirs = env.gen_obs()                 # (the first observation: BEFORE the session takes the state over)
        with env.persistent(max_steps=T) as ps:
            for t in range(T):
                obs, dirs, reward, terminated, truncated = ps.step(policy(obs))      # == env.step(...) bit for bit

    `ps.step(a)` = `ps.post(a)` (the actions, stream-ordered behind the policy that produced them) + `ps.wait()` (work enqueued on
    the current stream afterwards sees the step's outputs in the env's output buffers).  The env's own `step()` / `rollout()` /
    state tensors are unavailable until the session is closed (the state lives in the launch).  Inside a session synchronise
    STREAMS (`torch.cuda.current_stream().synchronize()`, events), never the device: `torch.cuda.synchronize()` waits for the
    resident launch itself, which waits for the next actions -- until its timeout ends the session."""

    def __init__(self, env, max_steps: int, auto_reset: bool, timeout_ms: int):
        be = env.backend
        if not hasattr(be, "persistent_launch"):
            raise RuntimeError("persistent stepping needs the HIP backend")
        if auto_reset and getattr(env, "_gen", None) is not None:
            raise RuntimeError("persistent stepping restarts finished envs from a layout pool (set_layout_pool), not from the "
                               "device generator")
        self.env, self.max_steps, self.timeout_ms = env, int(max_steps), int(timeout_ms)
        self.auto_reset = bool(auto_reset)
        B, A, dev = env.batch, env.spec.num_agents, env.device
        self.waves = be.persistent_waves(B, self.auto_reset)
        self.granules = torch.zeros((B, (A + 3) // 4), dtype=torch.int64, device=dev)
        self.done = torch.zeros((self.waves,), dtype=torch.int32, device=dev)
        self.ctrl = torch.tensor([0, 0, 0, -1] + [0] * 4, dtype=torch.int32, device=dev)
        # a stream of its own, HIGH priority: the launch runs BESIDE whatever produces its actions (HIP multiplexes the streams of
        # one priority over a few hardware queues; the priorities have queues of their own, so no producer stream ever shares
        # one with the launch), and its few wavefronts are served first wherever they share a SIMD with the producer's
        self.stream = torch.cuda.Stream(dev, priority=-1)
        self.t = 0                       # steps posted
        self.waited = 0                  # steps waited for
        self.open = False
        ar = env._auto_reset_args(self.auto_reset, getattr(env, "was_reset", None))
        self._sa, self._keep = be.step_args(env._cells, env.agents, env.rng, env.step_count,
                                            env.aux if env.spec.env_kind != "empty" else None, env.err, env.obs, env.dir,
                                            env.reward, env.terminated, env.truncated, auto_reset=ar)
        self._pers = be.persistent_struct(self.granules, self.done, self.ctrl, self.max_steps, self.timeout_ms)

    def __enter__(self):
        env = self.env
        env._need_state()
        env.join()
        if env._session is not None:
            raise RuntimeError("this env already has a persistent session open")
        env._disarm()                                      # (the launch writes the grids back without keeping the layout marker)
        cur = torch.cuda.current_stream(env.device)
        self.stream.wait_stream(cur)                       # (the state and the zeroed hand-shake words are in place)
        env.backend.persistent_launch(env.batch, self._sa, self._pers, self.stream.cuda_stream)
        env._session = self
        self.open = True
        return self

    def post(self, actions: torch.Tensor):
        """Hand over the actions of the next step (i8[B,A] on the env's device), stream-ordered on the current stream."""
        env = self.env
        if not self.open or self.t >= self.max_steps:
            raise RuntimeError("the persistent session is closed or has used up its max_steps")
        if actions.dtype is not torch.int8 or actions.shape != env._act_shape or actions.device != env._cells.device \
                or not actions.is_contiguous():
            raise ValueError(f"actions must be a contiguous int8 tensor of shape {tuple(env._act_shape)} on {env._cells.device}")
        self.t += 1
        env.backend.persistent_post(env.batch, actions, self.t, self.granules)

    def wait(self):
        """Work enqueued on the current stream after this call sees the outputs of the last posted step."""
        self.env.backend.persistent_wait(self.done, self.waves, self.t, self.ctrl, self.timeout_ms)
        self.waited = self.t
        env = self.env
        return env.obs, env.dir, env.reward, env.terminated, env.truncated

    def step(self, actions: torch.Tensor):
        self.post(actions)
        return self.wait()

    def feed(self, actions: torch.Tensor, trace: bool = False):
        """A recorded action sequence i8[T,B,A] played through the closed-loop hand-shake by ONE resident workgroup
        (mgx_persistent_feed: the shortest producer there can be; benchmarks and tests).  Returns the trace tensor
        (i64[2T + 1], s_memrealtime ticks of 10 ns) or None.  The session's remaining steps must cover T."""
        env = self.env
        T = int(actions.shape[0])
        if self.t != 0 or T != self.max_steps:
            raise RuntimeError("feed() plays a whole session: max_steps == len(actions), nothing posted before")
        if actions.dtype is not torch.int8 or tuple(actions.shape[1:]) != tuple(env._act_shape) or not actions.is_contiguous():
            raise ValueError("actions must be a contiguous int8 tensor [T,B,A]")
        tr = torch.zeros((2 * T + 1,), dtype=torch.int64, device=env.device) if trace else None
        env.backend.persistent_feed(env.batch, actions, T, self._pers, self.waves, tr, torch.cuda.current_stream(env.device).cuda_stream)
        self.t = self.waited = T
        return tr

    def close(self):
        """End the launch (a stop request unless it has run all of its steps), join its stream: the env's state tensors hold
        the state after the last completed step.  Raises if a wait inside the launch timed out."""
        if not self.open:
            return
        env = self.env
        cur = torch.cuda.current_stream(env.device)
        if self.t < self.max_steps:
            if self.waited < self.t:
                self.wait()
            self.ctrl[0:1].fill_(1)                         # stop request, stream-ordered behind the last wait
        cur.wait_stream(self.stream)
        self.open = False
        env._session = None
        c = [int(v) & 0xFFFFFFFF for v in self.ctrl.cpu()]
        self.timeouts, self.waves_left, self.steps_completed = c[1], c[2], c[3]
        if c[1]:
            raise RuntimeError(f"persistent stepping: {c[1]} wait(s) timed out after {self.timeout_ms} ms "
                               f"(steps completed by every wavefront: {c[3]})")

    def __exit__(self, *exc):
        try:
            self.close()
        except RuntimeError:
            if exc[0] is None:
                raise
        return False

    def __del__(self):
        # a session dropped without close(): ask the launch to stop (it would otherwise wait out its timeout on the device); the env
        # stays marked as having a session -- its state tensors are only valid once somebody has joined the launch's stream
        try:
            if getattr(self, "open", False):
                self.ctrl[0:1].fill_(1)
        except Exception:               # noqa: BLE001  (interpreter shutdown, device gone: nothing to do)
            pass


class BatchedMultiGridEnv:
    def __init__(self, spec: EnvSpec, batch: int, device="cuda", *, first_env: int = 0, backend=None, specialise=None):
        """
        spec       environment class configuration
        batch      number of envs held by THIS process (its shard of the global batch)
        device     HIP device ('cuda', 'cuda:3', ...).  CPU devices are refused: there is no CPU path.
        first_env  global index of env 0 of this shard; per-env seeds are a function of the global index so
                   results do not depend on how the batch is sharded over GPUs
        backend    launcher override used by the test-suite to exercise this host logic without a GPU;
                   product code leaves it None (= ops.HipBackend).
        specialise True: compile a shape-specialised step kernel for this (spec, batch) at run time if the library has none built
                   in (multigrid_amd/jit.py: hipRTC, ~1-2 s once, cached on disk; 10-14 % of a step in the latency regime, same
                   results).  None (default): what the environment variable MGX_JIT says (unset / 0 = no).
        """
        self.spec = spec
        self.batch = int(batch)
        self.first_env = int(first_env)
        self.device = torch.device(device)
        if backend is None:
            from .ops import HipBackend
            backend = HipBackend(spec, self.device)
        self.backend = backend
        B, A, dev = self.batch, spec.num_agents, self.device
        # packed cells: MgxCell bit patterns (i16), or -- spec.cell_bytes == 1 -- the compact MgxCell8 bytes (include/mgx.h)
        # (spec.cell_bytes == 3: the reference's byte triples themselves, u8[B,H,W,3])
        self._cells = torch.zeros(spec.cells_shape(B), dtype=torch.uint8 if spec.cell_bytes != 2 else torch.int16, device=dev)
        # the layout marker (include/mgx.h: mgx_step_tracked): i32[B], k >= 0 = env b's cells equal layout k of the pool bit for bit,
        # -1 = unknown.  `_mark` is shared with the sub-shards of split(): "armed" = the marker may hold a k >= 0 (only then does a
        # path that writes cells behind its back pay the fill that takes the promise back: _disarm), "graphs" = a captured graph
        # holds tracked steps (it re-arms whenever it is replayed: "armed" then stays up), "root" = the whole tensor
        self._marker = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self._mark = {"armed": False, "graphs": False, "root": self._marker}
        self.agents = torch.zeros(spec.agents_shape(B), dtype=torch.uint8, device=dev)
        self.rng = torch.zeros((B, 4), dtype=torch.int64, device=dev)
        self.step_count = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.aux = torch.zeros((B, 16), dtype=torch.uint8, device=dev)       # the env subclass' hook state (include/mgx.h)
        # Everything a step hands back -- reward, obs, dir, terminated, truncated, the error words -- lies in ONE allocation (16-byte
        # aligned views of it), so that a host caller that wants all of it pays one device-to-host copy, not six (`outputs_to_host`:
        # the dict API, multigrid_amd/env.py; round 6)
        obs_shape = tuple(spec.obs_shape(B))
        parts = (("reward", torch.float64, (B, A)), ("obs", torch.uint8, obs_shape), ("dir", torch.uint8, (B, A)),
                 ("terminated", torch.uint8, (B, A)), ("truncated", torch.uint8, (B,)), ("err", torch.int32, (2,)))
        offs, total = {}, 0
        for name, dt, shape in parts:
            offs[name] = total
            total += (int(np.prod(shape)) * torch.empty((), dtype=dt).element_size() + 15) & ~15
        self._out = torch.zeros(max(total, 16), dtype=torch.uint8, device=dev)
        self._out_parts, self._out_host = [(n, dt, sh, offs[n]) for n, dt, sh in parts], None
        for name, dt, shape in parts:
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            setattr(self, name, self._out[offs[name]:offs[name] + nbytes].view(dt).view(shape))
        self.err.copy_(torch.tensor([0, INT32_MAX], dtype=torch.int32))
        self._loaded = False
        self._seeded = False             # np_random holds generator words (seed / seed_synthetic / load_state(rng=) / reset(seed))
        self._act_shape = torch.Size((B, A))
        self._bound = {}                 # (auto_reset, one_hot, generate[, parts]) -> pre-bound step launcher (ops.HipBackend)
        self._layout_version = 0         # bumped whenever the layout pool / generator tensors are REPLACED: sub-shards and
        self._parent = None              # captured graphs made before hold pointers into the old ones and refuse to run
        self._chain_streams = []         # side streams of the eager sub-shard form (step(..., sub_shards=P))
        self._chains_pending, self._chains_P = False, 1
        self._session = None             # an open PersistentSession: the state lives in its launch
        self._stats = None               # EpisodeStats while track_episodes() is on
        self._layout_epoch = 0           # bumped whenever the layouts the marker's indices name change (an in-place refill included)
        self._copy_bad = None            # i32[2]: the pairs snapshot() / restore() skipped (out of range), the first of them
        self.shape_kernel = None
        if specialise is None:
            specialise = os.environ.get("MGX_JIT", "0") not in ("", "0")
        if specialise and self.device.type == "cuda" and getattr(self.backend, "name", "") == "hip":
            self.specialise()

    def specialise(self) -> str:
        """Run this env's step on a kernel compiled for exactly its shape (multigrid_amd.jit.ensure_shape).  Returns what happened:
        "built-in" / "registered" / "compiled" / "not-latency" / "unavailable" (also kept in `.shape_kernel`)."""
        from . import jit
        self.shape_kernel = jit.ensure_shape(self.spec, self.batch, self.device)
        return self.shape_kernel

    @property
    def cells(self) -> torch.Tensor:
        """The packed grid cells (i16[B,H,W]; u8 for the compact / byte formats) -- the env's own tensor, for callers that read or
        WRITE it in place (the torch ops, a cell edit).  Handing it out takes back everything the layout marker promises about it
        (one fill, and only while the marker is armed): write through a reference taken earlier than the last `step()` and the
        next step may not see it.  The env's own methods use `_cells`."""
        self._disarm()
        return self._cells

    # ------------------------------------------------------------------------------------------ layout marker
    def _tracks(self) -> bool:
        """The steps of this env can keep the layout marker: 16-bit cells, restarts from a layout pool."""
        return getattr(self, "_pool", None) is not None and getattr(self, "_gen", None) is None and self.spec.cell_bytes == 2

    def _disarm(self):
        """Something is about to write cells without keeping the marker (a rollout, a persistent launch, a step without
        auto-reset, a torch op on `cells`, ...): nothing is known about any env's grid any more.  No kernel unless armed."""
        m = self._mark
        if m["armed"]:
            m["root"].fill_(-1)
            # (while a graph is captured the fill is only recorded, and a captured graph of tracked steps re-arms whenever it is
            # replayed: the flag then stays up)
            if not m["graphs"] and not (self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
                m["armed"] = False

    def _tracked_step(self):
        """A step that keeps the marker is about to be issued: its restarts arm it.  Captured into a graph, it does so again on
        every replay, whatever the host does in between."""
        m = self._mark
        if not m["graphs"]:
            m["armed"] = True
            if torch.cuda.is_current_stream_capturing():
                m["graphs"] = True

    def _arm(self):
        """The cells or the pool were replaced: compare once, on the device.  One layout: every env that equals it is marked 0;
        more: everything starts unknown, and the restarts mark the envs as they go."""
        if not self._tracks() or self._pool[0].shape[0] != 1:
            self._disarm()
            return
        same = (self._cells == self._pool[0][0]).flatten(1).all(dim=1)
        self._marker.copy_(same.to(torch.int32) - 1)
        self._mark["armed"] = True

    def _restarted(self):
        """reset_done() / reset() restarted the envs of `was_reset` from the pool: with one layout they ARE that layout now; with
        more, their marker would name the layout they had before -- unknown."""
        if self._tracks() and (self._mark["armed"] or self._pool[0].shape[0] == 1):
            one = self._pool[0].shape[0] == 1
            self._marker.masked_fill_(self.was_reset.bool(), 0 if one else -1)
            if one:
                self._mark["armed"] = True

    @property
    def grid(self) -> torch.Tensor:
        """The grid as (type, color, state) bytes u8[B,H,W,3] ([y][x]: layouts.grid_from_product gives the reference's
        Grid.state) -- unpacked from `cells` on every access; for inspection, tests and checkpoints, not the hot path.  A box that
        holds something carries it in the upper bits of its state byte (include/mgx.h "BOX CONTENTS"; `& 3` is what Grid.state
        shows)."""
        if self.spec.cell_bytes == 3:
            return self._cells
        c = self._cells.to(torch.int32)
        if self.spec.cell_bytes == 1:                        # MgxCell8: joint (type, state) code | color << 4 | opaque << 7
            tc = c & 0xF
            door = (tc == 11) | (tc == 12)
            t = torch.where(tc <= 10, tc, torch.where(door, torch.full_like(tc, 4), torch.full_like(tc, 10)))
            st = torch.where(tc <= 10, torch.zeros_like(tc), torch.where(door, tc - 10, tc - 12))
            return torch.stack((t, (c >> 4) & 0x7, st), dim=-1).to(torch.uint8)
        content = ((c >> 4) & 0xF) | (((c >> 11) & 1) << 4) | (((c >> 14) & 1) << 5)      # a box's content (include/mgx.h)
        return torch.stack((c & 0xF, (c >> 8) & 0x7, ((c >> 12) & 0x3) | (content << 2)), dim=-1).to(torch.uint8)

    # ------------------------------------------------------------------------------------------ state in
    def load_state(self, grid, agents, rng=None, aux=None, step_count=None, validate: bool = True, target=None):
        """Install an initial state (numpy arrays or tensors in the product layout).  A single env's state
        (no batch dim) is broadcast to the whole batch.  This is also the parity-injection point: the
        reference's `Grid.state` / `AgentState` go through layouts.grid_to_product / pack_agents."""
        self._no_session("load_state")
        sp, B = self.spec, self.batch

        def prep(x, shape, dtype):
            t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
            if t.dim() == len(shape) - 1:
                t = t.unsqueeze(0).expand(shape)
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
            return t.to(dtype=dtype).contiguous()

        self.join()
        g = prep(grid, sp.grid_shape(B), torch.uint8)
        a = prep(agents, sp.agents_shape(B), torch.uint8)
        if validate:
            layouts.check_walled(g.cpu().numpy() if g.device.type != "cpu" else g.numpy())
            an = a.cpu().numpy()
            if (an[..., 2] >= sp.width).any() or (an[..., 3] >= sp.height).any() or (an[..., 1] > 3).any():
                raise ValueError("agent position / direction out of range")
        self._refuse_carried_contents(a)
        self._cells.copy_(torch.from_numpy(layouts.pack_cells_for(sp, g.cpu().numpy())))
        self._arm()
        self.agents.copy_(a)
        if rng is not None:
            r = np.asarray(rng.cpu() if torch.is_tensor(rng) else rng)
            if r.dtype == np.uint64:
                r = r.view(np.int64)
            self.rng.copy_(prep(r, (B, 4), torch.int64))
            self._seeded = True
        if aux is None and target is not None:                 # BlockedUnlockPickup convenience: (type, color, state[, 0])
            t = np.zeros(np.asarray(target).shape[:-1] + (16,), dtype=np.uint8)
            t[..., :min(4, np.asarray(target).shape[-1])] = np.asarray(target)[..., :4]
            aux = t
        if aux is not None:
            self.aux.copy_(prep(aux, (B, 16), torch.uint8))
        elif self.spec.env_kind != "empty":
            raise ValueError(f"env_kind {self.spec.env_kind!r} needs `aux` (the env's hook state, include/mgx.h)")
        if step_count is None:
            self.step_count.zero_()
        else:
            self.step_count.copy_(prep(step_count, (B,), torch.int32))
        self._reset_err()
        self._state_written()
        self._loaded = True
        if self._stats is not None:
            self._rebase_episodes()

    def _refuse_carried_contents(self, agent_rows):
        """Compact cells (EnvSpec.cell_bytes = 1) have no room for what a box holds (include/mgx.h: MgxCell8): a filled box on the
        GRID is refused by the packer; one in an agent's HANDS (carry state byte >> 2, include/mgx.h "BOX CONTENTS") would lose its
        content when it is put down -- refused here, so that both formats give the same results or an error."""
        if self.spec.cell_bytes == 1:
            rows = agent_rows.cpu().numpy() if torch.is_tensor(agent_rows) else np.asarray(agent_rows)
            if (rows[..., 7] >> 2).any():
                raise ValueError("compact cells (cell_bytes = 1) cannot hold a box's content: an agent carries a filled box; "
                                 "use cell_bytes = 2 for envs with Box(contains=...)")

    def seed(self, seed: int):
        """Per-env `np_random = Generator(PCG64(SeedSequence([seed, global_env_index])))`; global env 0 gets
        `SeedSequence(seed)`, exactly what `gym.Env.reset(seed=seed)` gives the reference's single env
        (multigrid/base.py:269).  Keyed on the pair so that consecutive experiment seeds share no stream (seed + index
        would give env b under seed s+1 the stream of env b+1 under seed s), and a pure function of the GLOBAL env index
        so that sharding does not change any env's stream."""
        self._no_session("seed")
        self.join()
        idx = self.first_env + np.arange(self.batch)
        self.rng.copy_(torch.from_numpy(rnglib.words_from_seed_and_index(seed, idx).view(np.int64)))
        self._seeded = True
        self._state_written()

    def seed_synthetic(self, seed: int):
        """Benchmark-grade seeding: valid PCG64 states from a hash of the global env index (fast for large B)."""
        self._no_session("seed_synthetic")
        self.join()
        words = rnglib.synthetic_words(self.batch, seed, self.first_env)
        self.rng.copy_(torch.from_numpy(words.view(np.int64)))
        self._seeded = True
        self._state_written()

    def _reset_err(self):
        self.err.copy_(torch.tensor([0, INT32_MAX], dtype=torch.int32))

    def _state_written(self):
        """The env state (np_random, step counts, grids) was replaced from outside: what the staged generator prepared from the
        old state is void (the slots are a cache: dropping them is always valid), and nothing of the old state is in flight."""
        st = (getattr(self, "_gen", None) or {}).get("stage")
        if st is not None and st.get("candidates"):
            st["tag"].fill_(-1)
        elif st is not None:
            st["tag"][:, 0] = -1
            st["tag"][:, 3] = 0

    # ------------------------------------------------------------------------------------------ hot path
    def gen_obs(self, one_hot: bool = False):
        """multigrid/base.py:348-376 for every env: returns (obs u8[B,A,v,v,3], dir u8[B,A]).
        one_hot=True: the observation comes out one-hot encoded, u8[B,A,v,v,21] (`OneHotObsWrapper`,
        multigrid/wrappers.py:158-190), written by the same kernel launch; `obs` is not touched."""
        self._need_state()
        self.join()
        if one_hot:
            if self.spec.cell_bytes == 1:          # compact cells: the one-hot STEP is one launch (round 6); the observation of a
                self.backend.gen_obs(self.batch, self._cells, self.agents, self.obs, self.dir)      # reset is two: gen_obs, then
                self.backend.one_hot(self.obs, self._one_hot_buffer())                             # the one-hot kernel over it
                return self._one_hot, self.dir
            self._need_wide_cells("one-hot output")
            self.backend.gen_obs(self.batch, self._cells, self.agents, self._one_hot_buffer(), self.dir, one_hot=True)
            return self._one_hot, self.dir
        self.backend.gen_obs(self.batch, self._cells, self.agents, self.obs, self.dir)
        return self.obs, self.dir

    def _one_hot_buffer(self):
        if getattr(self, "_one_hot", None) is None:
            self._one_hot = torch.zeros(tuple(self.obs.shape[:-1]) + (21,), dtype=torch.uint8, device=self.device)
        return self._one_hot

    def _auto_reset_args(self, auto_reset, was_reset):
        if not auto_reset:
            return None
        if getattr(self, "_pool", None) is None:
            raise RuntimeError("auto_reset needs set_layout_pool() first")
        return (self.first_env, self._pool, self.episode, was_reset)

    def step(self, actions: torch.Tensor, auto_reset: bool = False, one_hot: bool = False, hook_order=None, sub_shards=1):
        """multigrid/base.py:303-346 for every env.

        one_hot=True: the first element returned is the one-hot observation u8[B,A,v,v,21] (what RLlib's default
        `OneHotObsWrapper` registration feeds the policy, multigrid/rllib/__init__.py:110-111), produced by the same launch
        (mgx_step_one_hot); the 3-channel `obs` buffer is not written.

        auto_reset=True fuses `reset_done()` into the launch (build-defined, include/mgx.h mgx_step_autoreset): an env
        whose episode ended with the previous step first restarts from the layout pool, then takes this step's
        actions; `was_reset` tells which ones did.  Bit-identical to `reset_done(); step(actions)`.

        actions     i8[B,A] on the env's device; `Action` values 0..6, NO_ACTION (-1) = agent not acting
                    (its key absent from the reference's actions dict, base.py:403-404).
        hook_order  u8[B,A] or None: per env, agent indices in the insertion order of the caller's actions dict -- the order
                    in which the RedBlueDoors / LockedHallway step hooks visit the agents (`for agent_id, action in
                    actions.items()`, multigrid/envs/redbluedoors.py:176, locked_hallway.py:210).  None = ascending index.
        sub_shards  1 (default): one launch for the whole batch on the current stream.  "auto" = `sub_shards_hint(form="eager")`,
                    which is 1 (per-step calls from Python are host-bound as chains); P > 1: the step is issued as P launches over consecutive blocks
                    of the batch on P side streams (mgx_step_chains) and is NOT joined -- consecutive calls form P independent
                    chains, so one block's load phase runs under another's compute (C4: 20.9 -> ~16 us per step).  The
                    outputs / state are complete after `join()`; any other method of this object joins first.  Same
                    results bit for bit (envs are independent; seeds and layouts follow the global env index).
        Returns (obs, dir, reward, terminated, truncated) -- the env's output buffers.
        An unknown action value does not raise here (no device sync on the hot path); it is recorded in
        `err` and surfaced as ValueError by `check_errors()` (multigrid/base.py:473-474).
        """
        if not self._loaded or self._session is not None:
            self._need_state()
        if self._parent is not None:
            self._check_fresh()
        if actions.dtype is not torch.int8 or actions.shape != self._act_shape or actions.device != self._cells.device \
                or not actions.is_contiguous():
            raise ValueError(f"actions must be a contiguous int8 tensor of shape {tuple(self._act_shape)} "
                             f"on {self._cells.device}")
        if sub_shards == 1 and hook_order is None and not self._chains_pending:      # the hot path: one dict lookup, one call
            fast = self._bound.get((auto_reset, one_hot))
            if fast is not None:
                if fast[2]:
                    self._tracked_step()
                elif self._mark["armed"]:
                    self._disarm()
                fast[0](actions)
                return fast[1]
        if hook_order is not None and (hook_order.dtype is not torch.uint8 or hook_order.shape != self._act_shape
                                       or hook_order.device != self._cells.device or not hook_order.is_contiguous()):
            raise ValueError(f"hook_order must be a contiguous uint8 tensor of shape {tuple(self._act_shape)} on {self._cells.device}")
        if one_hot and not (self.spec.cell_bytes == 1 and self.spec.env_kind == "empty"):
            self._need_wide_cells("one-hot output")        # (compact cells: the hook-free step has a one-hot instantiation, round 6)
        generate = bool(auto_reset) and getattr(self, "_gen", None) is not None
        if generate:
            # on-device generation: the envs whose episode ends with THIS step are regenerated right after it (in the tail
            # of the same launch when the launcher can: mgx_step_generate); `was_reset` = the envs regenerated by this call
            auto_reset = False
        P = 1
        if sub_shards != 1:
            P = self.sub_shards_hint(auto_reset or generate, one_hot, form="eager") if sub_shards == "auto" else int(sub_shards)
            P = max(1, min(P, self.batch // self.SUB_SHARD_ALIGN))
        if P > 1 and self._stats is not None:
            raise RuntimeError("episode accounting (track_episodes) does not follow an eager step(sub_shards=P > 1): its chains run "
                               "on side streams; capture_steps(sub_shards=P) is the supported form")
        if self._chains_pending and P != self._chains_P:       # (another cut of the batch over other streams: join the old chains)
            self.join()
        key = (bool(auto_reset), bool(one_hot), generate, P)
        if one_hot:
            self._one_hot_buffer()
        fast = self._bound.get(key)
        if fast is None:
            fast = self._bind_step(*key)
        out = (self._one_hot if one_hot else self.obs), self.dir, self.reward, self.terminated, self.truncated
        tracked = fast is not False and getattr(fast, "tracked", False)
        if tracked:
            self._tracked_step()
        else:                                   # (chains, one-hot, generated and plain steps, host launchers: the marker is not kept)
            self._disarm()
        if fast is not False:
            if P > 1:
                ev = self._fork_event
                ev.record(torch.cuda.current_stream(self.device))
                fast(actions, ev.cuda_event, hook_order)
                # the chains read `actions` / `hook_order` on their own streams and are not joined: the caching allocator must
                # not hand a temporary's block to the next allocation of the current stream while they still read it
                for st in self._chain_streams[:P]:
                    actions.record_stream(st)
                    if hook_order is not None:
                        hook_order.record_stream(st)
                self._chains_pending, self._chains_P = True, P
                return out
            if isinstance(auto_reset, bool) and isinstance(one_hot, bool):
                self._bound[(auto_reset or generate, one_hot)] = (fast, out, tracked)   # (the hot path's entry: cleared with _bound)
            fast(actions, hook_order)
            return out
        # launchers without bind_step (the test-suite's oracle backend)
        sp = self.spec
        ar = self._auto_reset_args(auto_reset, getattr(self, "was_reset", None))
        kw = {}
        if ar is not None:
            kw["auto_reset"] = ar
        if one_hot:
            kw["one_hot"] = True
        if hook_order is not None:
            kw["hook_order"] = hook_order
        obs = self._one_hot_buffer() if one_hot else self.obs
        self.backend.step(self.batch, self._cells, self.agents, self.rng, self.step_count, actions,
                          self.aux if sp.env_kind != "empty" else None, self.err,
                          obs, self.dir, self.reward, self.terminated, self.truncated, **kw)
        if self._stats is not None:
            self.backend.episode_stats(self.batch, 1, self.reward, self.terminated, self.truncated, self.was_reset if ar else None,
                                       _lib.RESTART_BEFORE if ar else _lib.RESTART_NONE, self._stats.tensors)
        if generate:
            self.reset_done()        # (with the accounting's restart clause behind it: together RESTART_AFTER)
        return obs, self.dir, self.reward, self.terminated, self.truncated

    def join(self):
        """Make torch's current stream wait for the sub-shard chains started by `step(..., sub_shards=P)`: afterwards work
        enqueued on the current stream sees every block's outputs and state.  (No host synchronisation.)"""
        if self._chains_pending:
            cur = torch.cuda.current_stream(self.device)
            for st in self._chain_streams:
                cur.wait_stream(st)
            self._chains_pending = False

    def sub_shards_hint(self, auto_reset: bool = False, one_hot: bool = False, form: str = "graph") -> int:
        """How many independent chains this env's step is best issued as on its device.

        form="graph" (`capture_steps(sub_shards="auto")`): mgx_sub_shards -- 1 when a launch is less than two wavefronts per
        SIMD, else 2, from the kernel's occupancy and the device's CU count, not from constants (C4: 18.6 -> 16.0-16.7 us per step).
        form="eager" (`step(sub_shards="auto")`): 1.  Issued per step from Python, P launches + P event waits + the allocator's
        stream bookkeeping cost the host more than a step lasts (C4, two chains: 32 us per step, host-bound, against 18.7 us as one
        launch: profiles/r5_bench.json `eager.c4_chains`, rounds 3-5 alike), so the chains only pay where the host is out of the
        loop -- in a captured graph.  An explicit `step(sub_shards=P)` is still honoured."""
        if form not in ("graph", "eager"):
            raise ValueError("form must be 'graph' or 'eager'")
        if form == "eager":
            return 1
        hint = getattr(self.backend, "sub_shards", None)
        if hint is None:
            return 1
        generate = bool(auto_reset) and getattr(self, "_gen", None) is not None
        return hint(self.batch, bool(auto_reset), bool(one_hot), generate)

    def _bind_step(self, auto_reset: bool, one_hot: bool, generate: bool = False, parts: int = 1):
        """Resolve every pointer of the step call once (ops.HipBackend.bind_step / bind_chains); False when the launcher
        cannot."""
        key = (auto_reset, one_hot, generate, parts)
        bind = getattr(self.backend, "bind_step" if parts == 1 else "bind_chains", None)
        if bind is None:
            self._bound[key] = False
            return False
        ar = self._auto_reset_args(auto_reset, getattr(self, "was_reset", None))
        head = (self.batch,)
        if parts > 1:
            while len(self._chain_streams) < parts:
                self._chain_streams.append(torch.cuda.Stream(self.device))
            if getattr(self, "_fork_event", None) is None:
                self._fork_event = torch.cuda.Event()
                self._fork_event.record(torch.cuda.current_stream(self.device))     # (creates the handle)
            head = (self.batch, parts, self._chain_streams[:parts])
        # the step with auto-reset from a layout pool keeps the layout marker (mgx_step_tracked); every other form leaves it alone
        # and step() takes the promise back before it runs
        track = ar is not None and parts == 1 and not one_hot and not generate and self._tracks()
        f = bind(*head, self._cells, self.agents, self.rng, self.step_count,
                 self.aux if self.spec.env_kind != "empty" else None, self.err,
                 self._one_hot_buffer() if one_hot else self.obs, self.dir, self.reward, self.terminated, self.truncated,
                 auto_reset=ar, one_hot=one_hot,
                 **({"generate": (self._gen, self.episode, self.was_reset)} if generate else {}),
                 **({"marker": self._marker} if track else {}))
        if self._stats is not None and parts == 1:
            f = self._with_accounting(f, ar is not None, generate)
        self._bound[key] = f
        return f

    def _with_accounting(self, step, pool_restart: bool, generate: bool):
        """The step launcher and the accounting launch directly behind it on the same stream as ONE launcher: what a tracking env
        binds in place of the step's own, so that step()'s hot path stays one lookup and one call -- and an env that does not
        track pays nothing."""
        restart = _lib.RESTART_BEFORE if pool_restart else (_lib.RESTART_AFTER if generate else _lib.RESTART_NONE)
        account = self.backend.bind_episode_stats(self.batch, self.reward, self.terminated, self.truncated,
                                                  self.was_reset if restart != _lib.RESTART_NONE else None, restart, self._stats.tensors)

        def tracked_step(actions, hook_order=None):
            step(actions, hook_order)
            account()
        tracked_step._keep = (step, account)
        tracked_step.tracked = getattr(step, "tracked", False)
        return tracked_step

    def _check_fresh(self):
        """A sub-shard (or a captured graph) holds pointers into its parent's layout pool / generator tensors."""
        if self._parent is not None and self._parent._layout_version != self._made_version:
            raise RuntimeError("this sub-shard was split off before its parent's set_layout_pool() / set_layout_generator() "
                               "replaced the layout tensors (or track_episodes() the accounting's): split() / capture_steps() again")

    # ------------------------------------------------------------------------------------------ sub-shards
    SUB_SHARD_ALIGN = 64         # envs: keeps every sub-shard's tensors 16-byte aligned and its wavefronts' tiles as in the whole

    def split(self, parts: int) -> list:
        """`parts` sub-shards of this env: views over consecutive blocks of its tensors (nothing is copied; `first_env` follows,
        so seeds and auto-reset layouts stay functions of the global env index).  Envs are independent, so stepping the
        sub-shards -- in any interleaving, on any streams -- is stepping this env.  Call it after the state, the layout pool /
        generator and any one-hot use are set up (the views are taken of the tensors as they are now)."""
        self._need_state()
        self.join()
        B, al = self.batch, self.SUB_SHARD_ALIGN
        parts = max(1, min(int(parts), max(1, B // al)))
        cuts = [0] + [min(B, ((B * i // parts + al - 1) // al) * al) for i in range(1, parts)] + [B]
        out = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            if hi <= lo:
                continue
            c = object.__new__(BatchedMultiGridEnv)
            c.spec, c.batch, c.first_env, c.device, c.backend = self.spec, hi - lo, self.first_env + lo, self.device, self.backend
            for name in ("_cells", "agents", "rng", "step_count", "aux", "obs", "dir", "reward", "terminated", "truncated"):
                setattr(c, name, getattr(self, name)[lo:hi])
            c._marker, c._mark = self._marker[lo:hi], self._mark          # (its slice of the layout marker; one host flag for all)
            c.err = self.err                                                  # (shared: the kernels update it atomically)
            c._loaded, c._act_shape, c._bound = True, torch.Size((hi - lo, self.spec.num_agents)), {}
            c._parent, c._made_version, c._layout_version = self, self._layout_version, 0
            c._chain_streams, c._chains_pending, c._chains_P, c._session = [], False, 1, None
            c._seeded = self._seeded
            c._stats = self._stats._slice(lo, hi) if self._stats is not None else None
            c._one_hot = self._one_hot[lo:hi] if getattr(self, "_one_hot", None) is not None else None
            c._pool = getattr(self, "_pool", None)
            c._gen = None
            if getattr(self, "_gen", None) is not None:
                c._gen = dict(self._gen, gen_state=self._gen["gen_state"][lo:hi])
                if self._gen.get("stage") is not None:          # (its own slice of the staging slots, its own step count)
                    st = self._gen["stage"]
                    c._gen["stage"] = {k: (v[lo:hi] if torch.is_tensor(v) else v) for k, v in st.items()}
                    if st.get("external") and st.get("stream") is not None:
                        c._gen["stage"]["stream"] = torch.cuda.Stream(self.device)
                    c._gen["stage"]["phase"] = [st["phase"][0]]
            if getattr(self, "episode", None) is not None:
                c.episode, c.was_reset = self.episode[lo:hi], self.was_reset[lo:hi]
            c._range = (lo, hi)
            out.append(c)
        return out

    def capture_steps(self, actions: torch.Tensor, auto_reset: bool = False, one_hot: bool = False, sub_shards=1,
                      hook_order=None):
        """A hipGraph of `len(actions)` consecutive `step` launches reading `actions[t]` (i8[T,B,A], kept by reference: refill
        it between replays; `hook_order` u8[T,B,A] likewise).  `graph.replay()` then costs no Python per step; the outputs of
        the LAST step are in the env's buffers.  (A policy in the loop is captured the same way: see examples/closed_loop.py.)

        sub_shards=P > 1 or "auto" (`sub_shards_hint()`): the batch is stepped as P independent sub-shards (`split`), each a
        chain of T launches on its own stream -- P parallel branches of the one graph.  A launch that fills the chip in a
        single round of wavefronts first loads (no wave has data to work on), then computes, then drains, and the next launch of
        its chain cannot start before its last wave has gone; the chains drift apart and fill each other's bubbles (C4: 20.9 ->
        15.7 us per step of the whole batch, C5 85 -> 69 us; in-kernel timestamps of the overlap: profiles/r3_chain_overlap.txt).
        Same results: envs are independent.  This is the double-buffered actor loop of a closed-loop caller (policy on one block
        while the others step).  A policy that needs all B observations of step t before step t+1 uses sub_shards=1.

        Returns a StepGraph (`.replay()`, `.graph` = the torch.cuda.CUDAGraph, `.sub_shards`); it refuses to replay once
        set_layout_pool() / set_layout_generator() have replaced the tensors it captured pointers to."""
        self._need_state()
        self.join()
        if sub_shards == "auto":
            sub_shards = self.sub_shards_hint(auto_reset, one_hot)
        stream = torch.cuda.current_stream(self.device)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(stream)
        if one_hot:
            self._one_hot_buffer()
        shards = self.split(sub_shards) if sub_shards > 1 else [self]
        others = [torch.cuda.Stream(self.device) for _ in shards[1:]]
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                for s in others:                                             # fork
                    s.wait_stream(side)
                for i, sh in enumerate(shards):
                    lo, hi = getattr(sh, "_range", (0, self.batch))
                    with torch.cuda.stream(side if i == 0 else others[i - 1]):
                        st = (getattr(sh, "_gen", None) or {}).get("stage") if auto_reset else None
                        before = st.get("launches", 0) if st else 0
                        for t in range(actions.shape[0]):
                            ho = None if hook_order is None else (hook_order[t] if sh is self else hook_order[t, lo:hi])
                            sh.step(actions[t] if sh is self else actions[t, lo:hi], auto_reset=auto_reset, one_hot=one_hot,
                                    hook_order=ho)
                        # candidates (set_layout_generator): a block shorter than the generator launches' cadence may have caught
                        # none of them -- and would then never make a candidate, however often it is replayed: it ends with one
                        # (every shard makes the candidates of its own slice, on its own chain: ADVICE r5)
                        if st and st.get("candidates") and st.get("launches", 0) == before:
                            sh.backend.stage_generate(sh.batch, sh._gen, sh.rng, sh.episode)
                for i, sh in enumerate(shards):                              # (generator streams of side-staged envs: join)
                    gs = ((getattr(sh, "_gen", None) or {}).get("stage") or {}).get("stream")
                    if gs is not None:
                        (side if i == 0 else others[i - 1]).wait_stream(gs)
                for s in others:                                             # join
                    side.wait_stream(s)
        stream.wait_stream(side)
        sg = StepGraph(self, graph, len(shards), (shards, others, actions, hook_order))
        ent = shards[0]._bound.get((bool(auto_reset), bool(one_hot)))
        sg._tracked = bool(ent and ent[2])       # (its steps keep the layout marker; otherwise a replay takes the promise back first)
        return sg

    def rollout(self, actions: torch.Tensor, out: dict | None = None, auto_reset: bool = False, one_hot: bool = False) -> dict:
        """`T` consecutive `step`s in one kernel launch (env state stays in LDS between steps); bit-identical to
        calling `step(actions[t])` for t = 0..T-1.  For open-loop action sequences (random / scripted policies).

        actions  i8[T,B,A].  Returns {'obs': u8[T,B,A,v,v,3], 'dir', 'reward', 'terminated': [T,B,A],
        'truncated': u8[T,B]} (pass `out` to reuse buffers).  The env's own `obs`... buffers are not touched.
        auto_reset=True: finished envs restart from the layout pool before each step (as `step(auto_reset=True)`);
        the result then also holds 'was_reset': u8[T,B].  With a layout generator set (`set_layout_generator`) the envs whose
        episode ends with a step are regenerated on the device right after it instead, and the call is T launches of the
        step kernel (as T calls of `step(auto_reset=True)`).  one_hot=True: 'obs' is the one-hot observation u8[T,B,A,v,v,21]
        (multigrid/wrappers.py:158-190), written by the same launch."""
        self._need_state()
        generate = bool(auto_reset) and getattr(self, "_gen", None) is not None
        if not (self.spec.cell_bytes == 1 and self.spec.env_kind == "empty" and not one_hot and not generate):
            self._need_wide_cells("rollout (the steps of one launch)")      # (compact cells: the hook-free rollout, round 6)
        self.join()
        self._disarm()                          # (the rollout kernels write the grids back without keeping the layout marker)
        sp, B = self.spec, self.batch
        if actions.dtype != torch.int8 or actions.dim() != 3 or tuple(actions.shape[1:]) != (B, sp.num_agents) \
                or actions.device != self._cells.device or not actions.is_contiguous():
            raise ValueError(f"actions must be a contiguous int8 tensor of shape (T, {B}, {sp.num_agents}) on {self._cells.device}")
        T, A, v, dev = actions.shape[0], sp.num_agents, sp.view_size, self.device
        if out is None:
            out = {"obs": torch.empty((T, B, A, v, v, 21 if one_hot else 3), dtype=torch.uint8, device=dev),
                   "dir": torch.empty((T, B, A), dtype=torch.uint8, device=dev),
                   "reward": torch.empty((T, B, A), dtype=torch.float64, device=dev),
                   "terminated": torch.empty((T, B, A), dtype=torch.uint8, device=dev),
                   "truncated": torch.empty((T, B), dtype=torch.uint8, device=dev)}
        if auto_reset and "was_reset" not in out:
            out["was_reset"] = torch.empty((T, B), dtype=torch.uint8, device=dev)
        generate = bool(auto_reset) and getattr(self, "_gen", None) is not None
        if generate:        # episode starts generated on the device: the envs whose episode ends with step t are regenerated
            aux, oh = self.aux if sp.env_kind != "empty" else None, {"one_hot": True} if one_hot else {}          # right after it
            if T > 1 and out["obs"][0].numel() % 16 and hasattr(self.backend, "stage_generate"):
                # T launches of the one-step kernel, which writes its observations from a 16-byte aligned base: where a step's
                # observations are no multiple of 16 bytes (130 envs x 2 agents x 27) the [t] slices of `obs` are not aligned, and
                # the launcher refuses slice 1 with step 0 already taken.  Each step then writes an aligned buffer and is copied
                # into place; the generator launches between the steps keep their cadence (ops.HipBackend.bind_step).
                scratch, st = torch.empty_like(out["obs"][:1]), self._gen.get("stage")
                for t in range(T):
                    self.backend.rollout(B, 1, self._cells, self.agents, self.rng, self.step_count, actions[t:t + 1], aux, self.err,
                                         scratch, out["dir"][t:t + 1], out["reward"][t:t + 1], out["terminated"][t:t + 1],
                                         out["truncated"][t:t + 1], generate=(self._gen, self.episode, out["was_reset"][t:t + 1]), **oh)
                    out["obs"][t:t + 1].copy_(scratch)
                    if st is not None and st.get("external") == 2 and st["phase"][0] % max(1, int(st.get("lead", 2)) // 2) == 0:
                        self.backend.stage_generate(B, self._gen, self.rng, self.episode)
            else:
                self.backend.rollout(B, T, self._cells, self.agents, self.rng, self.step_count, actions, aux, self.err, out["obs"],
                                     out["dir"], out["reward"], out["terminated"], out["truncated"],
                                     generate=(self._gen, self.episode, out["was_reset"]), **oh)
            self._account_rollout(out, T, _lib.RESTART_AFTER)
            return out
        ar = self._auto_reset_args(auto_reset, out.get("was_reset"))
        self.backend.rollout(B, T, self._cells, self.agents, self.rng, self.step_count, actions,
                             self.aux if sp.env_kind != "empty" else None, self.err, out["obs"], out["dir"],
                             out["reward"], out["terminated"], out["truncated"],
                             **({"auto_reset": ar} if ar is not None else {}), **({"one_hot": True} if one_hot else {}))
        self._account_rollout(out, T, _lib.RESTART_BEFORE if ar is not None else _lib.RESTART_NONE)
        return out

    def _account_rollout(self, out: dict, T: int, restart: int):
        """The accounting of a rollout: ONE launch over its [T,...] outputs; with track_episodes(trace=True) the result also gains
        'episode_closed' u8[T,B], 'episode_return' f64[T,B,A] and 'episode_length' i32[T,B] (the closed episode's values at a closing
        step, zeros elsewhere)."""
        st = self._stats
        if st is None:
            return
        trace = None
        if st.trace:
            B, A, dev = self.batch, self.spec.num_agents, self.device
            for name, dt, shape in (("episode_closed", torch.uint8, (T, B)), ("episode_return", torch.float64, (T, B, A)),
                                    ("episode_length", torch.int32, (T, B))):
                if name not in out:
                    out[name] = torch.empty(shape, dtype=dt, device=dev)
            trace = {"closed": out["episode_closed"], "episode_return": out["episode_return"], "episode_length": out["episode_length"]}
        self.backend.episode_stats(self.batch, T, out["reward"], out["terminated"], out["truncated"],
                                   out["was_reset"] if restart != _lib.RESTART_NONE else None, restart, st.tensors, trace)

    # ------------------------------------------------------------------------------------------ episode accounting
    def track_episodes(self, trace: bool | None = False):
        """Keep the return, the length and the outcome of every episode on the device (include/mgx.h "EPISODE ACCOUNTING"): what
        gymnasium's RecordEpisodeStatistics, EnvPool's info["episode"] and gymnax' LogWrapper give their callers.  Returns the
        `EpisodeStats` (also `.episode_stats`); `track_episodes(None)` stops.

        From then on every stepping and restart form of this env issues the accounting launch itself, on the same stream, directly
        behind the launch it accounts for: `step()` (one extra launch per step; captured with it by `capture_steps()`, sub-shards
        included), `rollout()` (one launch over the T steps' outputs; trace=True: the result also holds 'episode_closed',
        'episode_return', 'episode_length' per step), `reset_done()` / `reset(seed, mask)` (a restarted env's running episode is
        counted as aborted), `load_state()` (every env restarts).  An episode ends where the step's OUTPUTS say so -- truncated,
        or every agent terminated.  An env whose episode is already over when tracking starts is skipped until it restarts.
        Sub-shards and graphs made before the call refuse to run.  Not available: `persistent()` (the state lives in the resident
        launch) and the eager `step(sub_shards=P > 1)` -- both raise while tracking is on."""
        self._no_session("track_episodes")
        self.join()
        self._bound.clear()              # (the launchers bound so far step without / with the accounting)
        self._layout_version += 1        # (sub-shards and captured graphs made before hold the other form)
        if trace is None:
            self._stats = None
            return None
        self._stats = EpisodeStats(self.batch, self.spec.num_agents, self.device, trace=bool(trace))
        if self._loaded:
            self._stats.over.copy_(self.is_done())
        return self._stats

    @property
    def episode_stats(self):
        """The `EpisodeStats` of `track_episodes()`, or None."""
        return self._stats

    def _rebase_episodes(self):
        """The whole state was replaced (load_state, the first reset): every env restarts, and one that is already over stays
        out of the books until it is restarted."""
        self.backend.episode_restart(self.batch, None, self._stats.tensors)
        self._stats.over.copy_(self.is_done())

    # ------------------------------------------------------------------------------------------ either side of the path
    def one_hot_obs(self) -> torch.Tensor:
        """`OneHotObsWrapper` (multigrid/wrappers.py:101-190) applied to the current `obs`: u8[B,A,v,v,21]."""
        self.join()
        self.backend.one_hot(self.obs, self._one_hot_buffer())
        return self._one_hot

    def full_obs(self) -> torch.Tensor:
        """`FullyObsWrapper` (multigrid/wrappers.py:17-58): u8[B,W,H,3], the grid in the reference's [x][y]
        orientation with every agent (terminated or not) drawn at its position."""
        self._need_state()
        self.join()
        if getattr(self, "_full", None) is None:
            self._full = torch.zeros((self.batch, self.spec.width, self.spec.height, 3), dtype=torch.uint8,
                                     device=self.device)
        try:
            self.backend.full_obs(self.batch, self._cells, self.agents, self._full)
        except _lib.MgxError as e:
            # mgx_full_obs stages one env's cells and output in 64 KiB of LDS: (cb + 3) * W * H + 96 bytes, which refuses sides
            # beyond 114 / 127 / 104 on 16-bit / compact / byte cells where the step runs up to 255.  Those
            # grids get the same tensor from the unpacked grid: transposed to [x][y], the state's box content masked off as in
            # Grid.state, every agent drawn over it in index order (multigrid/wrappers.py:52-54).
            if e.code != _lib.ERR_UNSUPPORTED:
                raise
            img = self.grid.permute(0, 2, 1, 3) & torch.tensor([255, 255, 3], dtype=torch.uint8, device=self.device)
            ag = self.agents.long()
            env = torch.arange(self.batch, device=self.device)
            for a in range(self.spec.num_agents):
                img[env, ag[:, a, 2], ag[:, a, 3]] = torch.stack(
                    (torch.full_like(ag[:, a, 0], int(Type.agent)), ag[:, a, 0], ag[:, a, 1]), dim=-1).to(torch.uint8)
            self._full.copy_(img)
        return self._full

    def render(self, env_ids=None, tile_size: int = 32, highlight: bool = True, out: torch.Tensor | None = None) -> torch.Tensor:
        """RGB frames, u8[N, H*tile_size, W*tile_size, 3] on the device: `MultiGridEnv.get_full_render(highlight, tile_size)`
        (multigrid/base.py:707-760) of every env, or of the envs `env_ids` (an integer tensor, e.g. a few envs of a big batch to
        log).  `highlight` shades the cells any agent sees, from a gen_obs of the state into a private buffer: the env's state and
        every buffer it has handed out (obs, dir, one-hot, reward, the flags) are left as they are.  `out`: a contiguous uint8
        tensor of that shape on this device to write into.  Tiles come from an atlas rendered once per (device, tile_size)."""
        self._no_session("render")
        self._need_state()
        self.join()
        ts = int(tile_size)
        if not 1 <= ts <= 64:
            raise ValueError(f"render: tile_size must be in 1..64, got {tile_size}")
        cells, agents = self._cells, self.agents
        if env_ids is not None:
            ids = torch.as_tensor(env_ids)
            if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
                raise TypeError(f"render: env_ids must be an integer tensor, got {ids.dtype}")
            if ids.dim() != 1:
                raise ValueError(f"render: env_ids must be one-dimensional, got shape {tuple(ids.shape)}")
            if ids.numel():
                lo, hi = (int(v) for v in torch.stack((ids.min(), ids.max())).tolist())
                if lo < 0 or hi >= self.batch:
                    raise ValueError(f"render: env_ids must lie in [0, {self.batch}), got {lo}..{hi}")
            ids = ids.to(device=self.device, dtype=torch.long)
            cells, agents = cells.index_select(0, ids), agents.index_select(0, ids)
        n, sp = cells.shape[0], self.spec
        shape = (n, sp.height * ts, sp.width * ts, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif (tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous()):
            raise ValueError(f"render: out must be a contiguous uint8 tensor of shape {shape} on {self.device}")
        if n == 0:
            return out
        obs = None
        if highlight:
            scratch = getattr(self, "_render_scratch", None)
            if scratch is None or scratch[0].shape[0] < n:
                scratch = (torch.empty((n,) + tuple(self.obs.shape[1:]), dtype=torch.uint8, device=self.device),
                           torch.empty((n, sp.num_agents), dtype=torch.uint8, device=self.device))
                self._render_scratch = scratch
            obs, dirs = scratch[0][:n], scratch[1][:n]
            self.backend.gen_obs(n, cells, agents, obs, dirs)
        self.backend.render(n, cells, agents, obs, ts, out)
        return out

    def render_views(self, obs: torch.Tensor | None = None, dir: torch.Tensor | None = None, *, env_ids=None, colors=None,
                     tile_size: int = 8, highlight: bool = True, channels_first: bool = False,
                     out: torch.Tensor | None = None) -> torch.Tensor:
        """Every agent's view as the RGB frame it sees, u8[..., A, P, P, 3] on the device with P = view_size * tile_size (or
        u8[..., A, 3, P, P] with `channels_first`, what a torch CNN takes): the partial pixel observation of MiniGrid's
        RGBImgPartialObsWrapper, by the rule of include/mgx.h "VIEW FRAMES" -- the viewer at the bottom centre facing up, other
        agents turned by the viewer's direction, the carried object under the viewer, unseen cells dark.  ONE launch.

        obs, dir   None: the env's own latest outputs, frames u8[B, A, ...].  Otherwise contiguous uint8 tensors [..., A, v, v, 3] and
                   [..., A] on the env's device -- a rollout's [T, B, A, ...] is one launch.
        colors     each viewer's own colour: a contiguous uint8 tensor of `dir`'s shape.  None: the env's agent colours u8[B, A], for
                   which the leading dimensions must end in [B, A].
        env_ids    instead of `obs`: a contiguous int64 [n] tensor on the env's device.  Those envs are observed into a private buffer
                   first, as render(highlight=True) does, so a restored or forked env is drawn without stepping it: frames
                   u8[n, A, ...].  Its form is checked, its values are not (no host round trip): an id outside [0, batch) is clamped
                   into the batch.
        highlight  shade every cell the agent sees; out: a contiguous uint8 tensor of the result's shape on this device to write into.
        The env's state and every buffer it has handed out are left as they are.  Tiles come from an atlas rendered once per (device,
        tile_size, layout): the first call for one renders it, every later call can be captured in a graph."""
        self._no_session("render_views")
        ts, sp = int(tile_size), self.spec
        if not 1 <= ts <= 64:
            raise ValueError(f"render_views: tile_size must be in 1..64, got {tile_size}")
        A, v = sp.num_agents, sp.view_size
        if (obs is None) != (dir is None):
            raise ValueError("render_views: obs and dir go together")
        if env_ids is not None:
            if obs is not None:
                raise ValueError("render_views: env_ids and obs exclude each other")
            self._need_state()
            self.join()
            ids = self._index_arg("render_views", "env_ids", env_ids).clamp(0, self.batch - 1)
            n = int(ids.shape[0])
            cells, agents = self._cells.index_select(0, ids), self.agents.index_select(0, ids)
            scratch = getattr(self, "_render_scratch", None)
            if scratch is None or scratch[0].shape[0] < n:
                scratch = (torch.empty((n,) + tuple(self.obs.shape[1:]), dtype=torch.uint8, device=self.device),
                           torch.empty((n, A), dtype=torch.uint8, device=self.device))
                self._render_scratch = scratch
            obs, dir = scratch[0][:n], scratch[1][:n]
            if n:
                self.backend.gen_obs(n, cells, agents, obs, dir)
            if colors is None:
                colors = agents[:, :, 0].contiguous()
        elif obs is None:
            self._need_state()
            self.join()
            obs, dir = self.obs, self.dir
        for name, t, tail in (("obs", obs, (A, v, v, 3)), ("dir", dir, (A,))):
            if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.device != self.device or not t.is_contiguous() \
                    or tuple(t.shape[-len(tail):]) != tail:
                raise ValueError(f"render_views: {name} must be a contiguous uint8 tensor [..., {', '.join(map(str, tail))}] on {self.device}")
        lead = tuple(dir.shape)
        if tuple(obs.shape[:-3]) != lead:
            raise ValueError(f"render_views: obs {tuple(obs.shape)} and dir {lead} disagree in their leading dimensions")
        if colors is None:
            if lead[-2:] != (self.batch, A):
                raise ValueError(f"render_views: the env's agent colours are [{self.batch}, {A}] and dir is {lead}: pass colors=")
            self._need_state()
            colors = self.agents[:, :, 0].contiguous()
        elif not torch.is_tensor(colors) or colors.dtype != torch.uint8 or colors.device != self.device \
                or not colors.is_contiguous() or tuple(colors.shape) != lead:
            raise ValueError(f"render_views: colors must be a contiguous uint8 tensor of dir's shape {lead} on {self.device}")
        P = v * ts
        shape = lead + ((3, P, P) if channels_first else (P, P, 3))
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != self.device
              or not out.is_contiguous()):
            raise ValueError(f"render_views: out must be a contiguous uint8 tensor of shape {shape} on {self.device}")
        n_views = dir.numel()
        if n_views:
            self.backend.render_views(n_views, obs, dir, colors, ts, bool(highlight), bool(channels_first), out)
        return out

    def set_layout_pool(self, grids, agents, auxs=None):
        """Pool of K pre-generated episode starts for `reset_done()`: u8[K,H,W,3], u8[K,A,8], u8[K,16] | None."""
        self._no_session("set_layout_pool")
        sp = self.spec
        g = torch.as_tensor(np.asarray(grids), dtype=torch.uint8)
        a = torch.as_tensor(np.asarray(agents), dtype=torch.uint8)
        K = g.shape[0]
        if tuple(g.shape) != (K, sp.height, sp.width, 3) or tuple(a.shape) != (K, sp.num_agents, 8) or K < 1:
            raise ValueError("layout pool has the wrong shape")
        layouts.check_walled(g.numpy())
        self._refuse_carried_contents(a)
        t = None
        if auxs is not None:
            t = torch.as_tensor(np.asarray(auxs), dtype=torch.uint8)
            if tuple(t.shape) != (K, 16):
                raise ValueError("layout pool aux must be u8[K,16]")
            t = t.to(self.device).contiguous()
        elif sp.env_kind != "empty":
            raise ValueError(f"env_kind {sp.env_kind!r} needs per-layout aux")
        self.join()
        cells = torch.from_numpy(layouts.pack_cells_for(sp, g.numpy()))
        old = getattr(self, "_pool", None)
        self._layout_epoch += 1          # (a snapshot's layout markers spoke of the old layouts)
        if (getattr(self, "_gen", None) is None and old is not None and old[0].shape == cells.shape and old[1].shape == a.shape
                and (old[2] is None) == (t is None)):
            # same shapes: refill the tensors in place -- sub-shards, pre-bound launchers and captured graphs stay valid
            old[0].copy_(cells); old[1].copy_(a)
            if t is not None:
                old[2].copy_(t)
            self.episode.zero_(); self.was_reset.zero_()
            self._arm()                  # (the layout marker spoke of the old layouts)
            return
        self._gen = None
        self._pool = (cells.to(self.device).contiguous(), a.to(self.device).contiguous(), t)
        self.episode = torch.zeros((self.batch,), dtype=torch.int32, device=self.device)
        self.was_reset = torch.zeros((self.batch,), dtype=torch.uint8, device=self.device)
        self._bound.clear()              # (the pre-bound launchers hold the old pool's pointers ...
        self._layout_version += 1        #  ... and so do sub-shards and captured graphs made before: they now refuse to run)
        self._arm()

    def set_layout_generator(self, kind: str, layout_seed: int = 0, *, room_size: int = 0, start=(1, 1, 0),
                             max_hallway_keys: int = 1, max_keys_per_room: int = 2, staged=True, lead: int | None = None):
        """Episode starts generated ON THE DEVICE (mgx_reset_generate) instead of picked from a host-made pool: every
        finished env runs the reference's own `_gen_grid` (rejection-sampling placement with numpy-compatible draws) in a
        kernel, one lane per env.

        kind         'empty_fixed' (EmptyEnv, agents at `start` = (x, y, dir)), 'empty_random' (EmptyEnv with
                     agent_start_pos=None), 'blockedunlockpickup' (`room_size`), 'redbluedoors' (the spec's 2*size x size grid),
                     'lockedhallway' (`room_size`, `max_hallway_keys`, `max_keys_per_room`; at most 16 rooms) or 'playground'
                     (`room_size`; at most 16 rooms) -- every env class of the reference
        layout_seed  seeds every env's placement generator: Generator(PCG64(SeedSequence([layout_seed, global index])))
        `reset_done()` then regenerates every finished env; `step(auto_reset=True)` regenerates the envs whose episode ends
        with that step right after it -- in the tail of the step's own launch (mgx_step_generate), so the returned
        observation is the terminal one and the state tensors already hold the next episode's start.
        staged       how the truncation resets -- known in advance -- are kept off the step's critical path (include/mgx.h: MgxGenStage;
                     same results bit for bit in every mode, the slots are a cache):
                       True (default) / "candidates"  EVERY episode end an adoption: the generators draw from env.np_random at most
                                    once (BlockedUnlockPickup: the door row; the others never), and the placement stream does not
                                    depend on when the episode ends -- so the next episode is generated while the current one runs,
                                    once per possible value of that draw (room_size - 2 <= 4 candidates), by one generator launch
                                    (mgx_stage_generate) every lead/2 steps between two steps; a step that ends an episode -- by
                                    truncation or by success / failure -- makes the draw and adopts the matching candidate (a copy).
                                    Playground (many draws) and room sizes above 6 fall back to "between"
                       "between"    `lead` steps before an env truncates its step takes a snapshot of np_random; every
                                    lead/2 steps ONE generator launch (mgx_stage_generate) between two steps serves the pending
                                    snapshots into per-env slots; the truncating step adopts its slot (a copy).  Measured at C3 with the
                                    episodes out of phase: 9.7 us per step, against 15.6 in-launch and 16.6 unstaged (pool: 7.3)
                       "side"       the same generator launches on a stream of their own beside the steps (a parallel branch of a
                                    captured graph): measured slower than "between" (14.2 us): the fork / join of the branches costs
                                    more than the generator's few microseconds every lead/2 steps
                       "in_launch"  round 3's form: generator wavefronts appended to every step's launch, two steps ahead
                       False        no staging: every finished env is generated in the tail of its step
                     (`step()` and `capture_steps()` issue the generator launches; `rollout()` does it inside mgx_step_ex)
        lead         steps between the snapshot and the truncation (default: max_steps / 4, at most 128; 2 for "in_launch");
                     "candidates": twice the number of steps between two generator launches (default: 2/3 of max_steps, at most 512)
        """
        self._no_session("set_layout_generator")
        sp = self.spec
        self._need_wide_cells("set_layout_generator (device-side episode generation)")
        if kind == "blockedunlockpickup":
            if sp.env_kind != "blockedunlockpickup" or (sp.width, sp.height) != (2 * room_size - 1, room_size):
                raise ValueError("blockedunlockpickup generator: the spec must be a BlockedUnlockPickup grid of (2*room_size-1) x room_size")
            blank = layouts.roomgrid_blank(room_size, 1, 2)
        elif kind == "redbluedoors":
            if sp.env_kind != "redbluedoors" or sp.width != 2 * sp.height:
                raise ValueError("redbluedoors generator: the spec must be a RedBlueDoors grid of (2*size) x size")
            blank = layouts.redbluedoors_blank(sp.height)
        elif kind == "lockedhallway":
            rs = int(room_size)
            if sp.env_kind != "lockedhallway" or rs < 4 or sp.width != 3 * (rs - 1) + 1 or (sp.height - 1) % (rs - 1):
                raise ValueError("lockedhallway generator: the spec must be 3 columns of `room_size` rooms")
            blank = layouts.lockedhallway_blank(2 * ((sp.height - 1) // (rs - 1)), rs)
        elif kind == "playground":
            rs = int(room_size)
            if sp.env_kind != "empty" or rs < 4 or (sp.width - 1) % (rs - 1) or (sp.height - 1) % (rs - 1):
                raise ValueError("playground generator: the spec must be a hook-free grid of `room_size` rooms")
            blank = layouts.roomgrid_blank(rs, (sp.height - 1) // (rs - 1), (sp.width - 1) // (rs - 1))
        elif kind in ("empty_fixed", "empty_random"):
            if sp.env_kind != "empty" or sp.width != sp.height:
                raise ValueError("empty generator: the spec must be a square Empty grid")
            blank = layouts.empty_blank(sp.width)
        else:
            raise ValueError(f"unknown layout generator {kind!r}")
        self.join()
        idx = self.first_env + np.arange(self.batch)
        self._gen = {"kind": kind, "room_size": int(room_size), "start": tuple(int(v) for v in start),
                     "max_hallway_keys": int(max_hallway_keys), "max_keys_per_room": int(max_keys_per_room),
                     "blank": torch.from_numpy(layouts.pack_cells(blank).view(np.int16)).to(self.device).contiguous(),
                     "gen_state": torch.from_numpy(rnglib.layout_gen_state(layout_seed, idx).view(np.int64)).to(self.device)}
        # candidates per env (include/mgx.h: MgxGenStage.candidates): one per value of the generator's single env.np_random draw
        cand = {"blockedunlockpickup": int(room_size) - 2, "redbluedoors": 1, "lockedhallway": 1, "empty_fixed": 1,
                "empty_random": 1}.get(kind, 0)
        if staged is True:
            staged = "candidates" if 1 <= cand <= 4 else "between"
        if staged not in (False, "candidates", "between", "side", "in_launch"):
            raise ValueError(f"staged must be True / 'candidates' / 'between' / 'side' / 'in_launch' / False, got {staged!r}")
        if staged == "candidates" and not 1 <= cand <= 4:
            raise ValueError(f"staged='candidates': the {kind!r} generator draws from env.np_random more than once (or has more than "
                             f"4 possible draws): use 'between'")
        if staged == "candidates" and sp.num_agents > 1:
            B, dev = self.batch, self.device
            # (here `lead` only sets the generator launches' cadence -- every lead/2 steps, by default a third of max_steps: a launch
            # costs 15-50 us of the stream's time whatever it finds to do (profiles/r5_candidates.txt), and an episode shorter than
            # the cadence merely generates in the tail of its last step.  Callers whose episodes are short pass a smaller `lead`.)
            lead = int(lead) if lead is not None else max(4, min(512, 2 * sp.max_steps // 3))
            lead = max(2, min(lead, sp.max_steps - 1))
            self._gen["stage"] = {"lead": lead, "external": 2, "stream": None, "candidates": cand,
                                  "grid": torch.zeros((B, cand, sp.height, sp.width), dtype=torch.int16, device=dev),
                                  "agents": torch.zeros((B, cand, sp.num_agents, 8), dtype=torch.uint8, device=dev),
                                  "aux": torch.zeros((B, cand, 16), dtype=torch.uint8, device=dev) if sp.env_kind != "empty" else None,
                                  "words": torch.zeros((B, cand, 6), dtype=torch.int64, device=dev),
                                  "tag": torch.full((B, 4), -1, dtype=torch.int32, device=dev), "phase": [0]}
        elif staged and sp.num_agents > 1:       # the staging slots: a cache, not state (tag -1 = empty)
            B, dev = self.batch, self.device
            tag = torch.zeros((B, 4), dtype=torch.int32, device=dev)
            tag[:, 0] = -1
            side = staged in ("side", "between")
            lead = int(lead) if lead is not None else (max(2, min(128, sp.max_steps // 4)) if side else 2)
            if not 2 <= lead < sp.max_steps or (side and lead < 4):
                side, lead, staged = False, 2, "in_launch"      # (episodes too short to look that far ahead: the in-launch form)
            self._gen["stage"] = {"lead": lead, "external": (2 if staged == "between" else 1) if side else 0, "stream": torch.cuda.Stream(dev) if side and staged == "side" and dev.type == "cuda" else None,
                                  "grid": torch.zeros((B, sp.height, sp.width), dtype=torch.int16, device=dev),
                                  "agents": torch.zeros((B, sp.num_agents, 8), dtype=torch.uint8, device=dev),
                                  "aux": torch.zeros((B, 16), dtype=torch.uint8, device=dev) if sp.env_kind != "empty" else None,
                                  "words": torch.zeros((B, 12), dtype=torch.int64, device=dev), "tag": tag, "phase": [0]}
        self._disarm()                   # (no pool: nothing keeps the layout marker any more)
        self._layout_epoch += 1
        self._pool = None
        self.episode = torch.zeros((self.batch,), dtype=torch.int32, device=self.device)
        self.was_reset = torch.zeros((self.batch,), dtype=torch.uint8, device=self.device)
        self._bound.clear()
        self._layout_version += 1        # (sub-shards and captured graphs made before hold the old tensors' pointers)

    def reset_done(self) -> torch.Tensor:
        """Vector-env auto-reset (build-defined; the reference leaves `if env.is_done(): env.reset()` to its caller):
        every finished env (multigrid/base.py:534-539) restarts from the layout pool, its `np_random` stream left
        running as an unseeded `reset()` does.  Returns was_reset u8[B].  Observations of the restarted envs are
        produced by the next `gen_obs()` / `step()`."""
        self._need_state()
        self.join()
        if getattr(self, "_gen", None) is not None:
            self.backend.reset_generate(self.batch, self._gen, self._cells, self.agents, self.rng, self.step_count,
                                        self.aux if self.spec.env_kind != "empty" else None, self.episode, self.was_reset)
            if self._stats is not None:
                self.backend.episode_restart(self.batch, self.was_reset, self._stats.tensors)
            return self.was_reset
        if getattr(self, "_pool", None) is None:
            raise RuntimeError("call set_layout_pool() or set_layout_generator() first")
        self.backend.reset_done(self.batch, self.first_env, self._pool, self._cells, self.agents, self.step_count,
                                self.aux, self.episode, self.was_reset)
        self._restarted()
        if self._stats is not None:
            self.backend.episode_restart(self.batch, self.was_reset, self._stats.tensors)
        return self.was_reset

    def reset(self, seed: int | None = None, mask: torch.Tensor | None = None, one_hot: bool = False):
        """`obs, info = env.reset(seed=seed)` of the reference (multigrid/base.py:250-301) for the envs the caller chooses, on the
        device: they start a new episode from the layout generator (`set_layout_generator`: the reference's own `_gen_grid`, draw
        for draw) or the layout pool (`set_layout_pool`), whether their episode is over or not.  Also the way to a FIRST episode:
        with nothing loaded yet, `reset()` of the whole batch is the initial state.

        seed     None: every np_random stream runs on, as an unseeded reset() leaves it (no host work at all).  An int: np_random of
                 the chosen envs is re-seeded with the restart by the rule `seed()` documents -- global env g gets
                 Generator(PCG64(SeedSequence([seed, g]))), global env 0 SeedSequence(seed) -- and the generation draws from that
                 fresh generator (the words are made on the host: one [B,4] copy to the device; only chosen envs take them).  The
                 placement generators of `set_layout_generator(layout_seed=...)` are never re-seeded: the reference's are made at
                 construction time, and its reset(seed) leaves them alone.
        mask     bool / uint8 [B] on the env's device: the envs to restart (None = all).  Read by the kernel as it is: no copy, no
                 host synchronisation.  Envs outside it keep every byte of their state -- a finished env stays finished.
        Returns `gen_obs(one_hot)` of the whole batch; `was_reset` holds the selection; reward / terminated / truncated are not
        touched.  The staging slots of a staged generator need no attention: a restart advances the env's episode counter, which
        is what makes a slot or a pending snapshot stale (include/mgx.h: MgxGenStage, tag != episode)."""
        self._no_session("reset")
        gen, pool = getattr(self, "_gen", None), getattr(self, "_pool", None)
        if gen is None and pool is None:
            raise RuntimeError("call set_layout_pool() or set_layout_generator() first")
        sel = None
        if mask is not None:
            self._need_state()
            if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (self.batch,) \
                    or mask.device != self._cells.device or not mask.is_contiguous():
                raise ValueError(f"mask must be a contiguous bool or uint8 tensor of shape ({self.batch},) on {self._cells.device}")
            sel = mask.view(torch.uint8) if mask.dtype is torch.bool else mask
        if seed is None and not self._loaded and not self._seeded:
            raise ValueError("reset(): np_random has never been seeded (all-zero PCG64 words are not a generator): pass seed=, or "
                             "call seed() / seed_synthetic() first")
        self.join()
        words = None
        if seed is not None:
            idx = self.first_env + np.arange(self.batch)
            words = torch.from_numpy(rnglib.words_from_seed_and_index(int(seed), idx).view(np.int64)).to(self.device)
        aux = self.aux if self.spec.env_kind != "empty" else None
        if gen is not None:
            side = (gen.get("stage") or {}).get("stream")
            if side is not None:                 # (generator launches beside the steps read gen_state / rng: behind them)
                torch.cuda.current_stream(self.device).wait_stream(side)
            self.backend.reset_generate_select(self.batch, gen, sel, words, self._cells, self.agents, self.rng, self.step_count,
                                               aux, self.episode, self.was_reset)
        else:
            self.backend.reset_select(self.batch, self.first_env, pool, sel, words, self._cells, self.agents, self.rng,
                                      self.step_count, self.aux, self.episode, self.was_reset)
            self._restarted()
        if seed is not None:
            self._seeded = True
        first, self._loaded = not self._loaded, True
        if self._stats is not None:
            if first:
                self._rebase_episodes()
            else:
                self.backend.episode_restart(self.batch, self.was_reset, self._stats.tensors)
        return self.gen_obs(one_hot)

    # ------------------------------------------------------------------------------------------ snapshot / restore / fork
    def _restart_source(self) -> tuple:
        """The kind of this env's restart source: ("none",), ("pool",) or ("gen", generator kind)."""
        if getattr(self, "_gen", None) is not None:
            return ("gen", self._gen["kind"])
        return ("pool",) if getattr(self, "_pool", None) is not None else ("none",)

    def _state_rows(self) -> dict:
        """This env as a state set (include/mgx.h: MgxEnvRows): every tensor that makes an env continue as it does -- the public
        state, and the three pieces of engine state beside it (the layout marker, the generator's words, the running episode)."""
        rows = {"cells": self._cells, "agents": self.agents, "rng": self.rng, "step_count": self.step_count, "aux": self.aux,
                "marker": self._marker}
        if self._restart_source() != ("none",):
            rows["episode"] = self.episode
        if getattr(self, "_gen", None) is not None:
            rows["gen_state"] = self._gen["gen_state"]
        if self._stats is not None:
            rows.update(cur_return=self._stats.cur_return, cur_length=self._stats.cur_length, over=self._stats.over)
        return rows

    def _copy_entry(self, what: str):
        self._no_session(what)
        self._need_state()
        if self._parent is not None:
            raise RuntimeError(f"{what}: this env is a sub-shard of split() -- a view of its parent's tensors; {what} on the parent")
        self._bad_words()
        self.join()

    def _row_set(self, what: str) -> RowSet:
        """This env's live tensors as the rows of a query (row_queries.py)."""
        self._copy_entry(what)
        # (`_cells`, not `cells`: reading the grid keeps the layout marker's promises)
        tensors = {"cells": self._cells, "agents": self.agents, "rng": self.rng, "step_count": self.step_count, "aux": self.aux}
        return RowSet(what, self, tensors, self.batch, self._cells.device, "env_ids")

    def _bad_words(self) -> torch.Tensor:
        """i32[2] on the device: how many pairs / keys / masks the copy, key and mask kernels skipped for an index out of range, and the
        first"""
        if self._copy_bad is None:
            self._copy_bad = torch.tensor([0, INT32_MAX], dtype=torch.int32).to(self.device)
        return self._copy_bad

    def _index_arg(self, what: str, name: str, t, check_below=None, distinct: bool = False):
        if not torch.is_tensor(t) or t.dtype is not torch.int64 or t.dim() != 1 or t.device != self._cells.device \
                or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous int64 tensor of shape (n,) on {self._cells.device}")
        if check_below is not None and t.numel():
            lo, hi = (int(v) for v in torch.stack((t.min(), t.max())).tolist())
            if lo < 0 or hi >= check_below:
                raise ValueError(f"{what}: {name} must lie in [0, {check_below}), got {lo}..{hi}")
            if distinct and int(torch.unique(t).numel()) != t.numel():
                raise ValueError(f"{what}: {name} names an env more than once")
        return t

    def snapshot(self, env_ids: torch.Tensor | None = None, out: EnvSnapshot | None = None) -> EnvSnapshot:
        """The state of the envs `env_ids` as an `EnvSnapshot`, taken on the device by ONE launch (mgx_env_copy) on the current
        stream: no host round trip, no synchronisation.  Row i of the snapshot is env env_ids[i].

        env_ids  a contiguous int64 [n] tensor on the env's device (None = every env, in order), read by the kernel as it is.  An
                 id outside [0, batch) is skipped, leaves its row as it was, and is reported by `check_errors()`.
        out      a snapshot of the same row count and members (one this env made before) to overwrite: a planner that snapshots
                 every step allocates nothing.
        See `restore()` for what a restored env is."""
        self._copy_entry("snapshot")
        src = self._state_rows()
        n = self.batch if env_ids is None else int(self._index_arg("snapshot", "env_ids", env_ids).shape[0])
        if out is not None:
            if not isinstance(out, EnvSnapshot) or out.spec != self.spec or out.rows != n or set(out.tensors) != set(src) \
                    or out.device != self._cells.device or out.source != self._restart_source():
                raise ValueError(f"snapshot: out= has another shape: it must be a snapshot of {n} row(s) of this env, with the members "
                                 f"{sorted(src)}")
            snap = out
        else:
            tensors = {m: torch.zeros((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for m, t in src.items()}
            snap = EnvSnapshot(self.spec, n, tensors, self._restart_source())
        snap._taken_from(self)
        self.backend.env_copy(n, src, self.batch, env_ids, snap.tensors, n, None, None, _lib.STAGE_NONE, False, self._copy_bad)
        return snap

    def restore(self, snap: EnvSnapshot, env_ids: torch.Tensor | None = None, rows: torch.Tensor | None = None,
                check: bool = False) -> None:
        """Put the envs `env_ids` back to rows of a snapshot, on the device, by ONE launch (mgx_env_copy) on the current stream:
        env env_ids[i] takes snapshot row rows[i].  The state tensors are written in place: pre-bound launchers and graphs from
        `capture_steps` stay valid (and a `torch.cuda.graph` may capture the call).  Outputs are not restored: `gen_obs()`.

        A restored env continues bit for bit as the env the row was taken from continued from the moment of the snapshot -- the
        grid, the agents, np_random, the step count, the hook state, and the engine state beside them (the layout marker, the
        running episode of `track_episodes()`):
          * with a layout generator this holds across episode ends too: the placement generator's words, np_random and the
            episode counter travel with the row (the staged generator's slots of the restored envs are dropped: a cache);
          * with a layout pool it holds up to the env's next restart.  From there the SLOT's own rule applies -- layout =
            (first_env + b + episode * 7919) mod K is a function of the slot b -- so forks of one source part at their first restart.

        env_ids  contiguous int64 [n] on the env's device (None = every env, in order); they must be distinct
        rows     contiguous int64 [n] (None = 0..n-1); rows may repeat: that is the fork
        check    True: the range of both and the distinctness of env_ids are verified with torch ops -- a synchronisation -- and
                 a ValueError names the fault.  False (default) trusts the caller: a pair out of range is skipped whole and
                 reported by `check_errors()`; the result of a duplicate env id is unspecified.
        The snapshot may come from another env object of equal spec and equal restart source (its layout markers then come out
        unknown).  A snapshot without the running episode restored into a tracking env starts a fresh episode there; nothing is
        counted as aborted."""
        self._copy_entry("restore")
        if not isinstance(snap, EnvSnapshot):
            raise TypeError("restore: not an EnvSnapshot")
        if snap.spec != self.spec:
            raise ValueError("restore: the snapshot was taken from an env of a different EnvSpec")
        if snap.source != self._restart_source():
            raise ValueError(f"restore: the snapshot's restart source {snap.source} differs in kind from this env's "
                             f"{self._restart_source()} (layout generator kind / layout pool / none)")
        if snap.device != self._cells.device:
            raise ValueError(f"restore: the snapshot lives on {snap.device}, this env on {self._cells.device}")
        if env_ids is not None:
            self._index_arg("restore", "env_ids", env_ids, self.batch if check else None, distinct=True)
        if rows is not None:
            self._index_arg("restore", "rows", rows, snap.rows if check else None)
        n = self.batch if env_ids is None else int(env_ids.shape[0])
        if rows is not None and int(rows.shape[0]) != n:
            raise ValueError(f"restore: rows has {int(rows.shape[0])} entries for {n} env(s): env_ids[i] takes snapshot row rows[i]")
        if rows is None and n > snap.rows:
            raise ValueError(f"restore: {n} env(s) to restore, the snapshot holds {snap.rows} row(s): pass rows=")
        gen = getattr(self, "_gen", None)
        st = (gen or {}).get("stage")
        if st is not None and st.get("stream") is not None:      # (generator launches beside the steps read gen_state / rng: behind them)
            torch.cuda.current_stream(self.device).wait_stream(st["stream"])
        tag, mode = None, _lib.STAGE_NONE
        if st is not None:
            tag, mode = st["tag"], (_lib.STAGE_CANDIDATES if st.get("candidates") else _lib.STAGE_SNAPSHOTS)
        keep = snap._is_of(self)             # (only there do the snapshot's layout indices name this env's layouts)
        if keep and snap._armed:             # markers >= 0 may be written -- by every replay, when a graph captures the call
            m = self._mark
            if not m["graphs"]:
                m["armed"] = True
                if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                    m["graphs"] = True
        self.backend.env_copy(n, snap.tensors, snap.rows, rows, self._state_rows(), self.batch, env_ids, tag, mode, not keep,
                              self._copy_bad)
        self._seeded = self._seeded or snap._seeded

    def fork(self, src_ids: torch.Tensor, dst_ids: torch.Tensor, check: bool = False) -> None:
        """Copy the state of env src_ids[i] into env dst_ids[i] (contiguous int64 [n] tensors on the env's device; sources may
        repeat, destinations must be distinct): `restore(snapshot(src_ids), dst_ids)`, two launches through a snapshot of n rows --
        so a destination may also be somebody's source.  `check` as in `restore()`."""
        self._copy_entry("fork")
        self._index_arg("fork", "src_ids", src_ids, self.batch if check else None)
        self._index_arg("fork", "dst_ids", dst_ids)
        if src_ids.shape[0] != dst_ids.shape[0]:
            raise ValueError(f"fork: {int(src_ids.shape[0])} source(s) for {int(dst_ids.shape[0])} destination(s)")
        self.restore(self.snapshot(src_ids), dst_ids, check=check)

    # ------------------------------------------------------------------------------------------ state / observation keys
    def state_key(self, env_ids: torch.Tensor | None = None, *, salt: int = 0, step_count: bool = False, rng: bool = False,
                  out: torch.Tensor | None = None) -> torch.Tensor:
        """A 64-bit key of the state of the envs `env_ids` (include/mgx.h "STATE KEYS"): int64 [n] on the device, made by ONE launch
        (mgx_state_key) on the current stream that reads the state once -- no host round trip, no synchronisation, capturable in a
        graph.  Equal states have equal keys; different ones differ but for a 2^-64 chance, so `torch.unique(keys)` dedups forked
        envs, a sort counts visits, and a search has its transposition key.

        The key covers what the reference shows of an env -- the grid (as `.grid` shows it, a box's content included), the agent
        rows and the hook state `aux` -- and, on request, `step_count` and np_random (`rng`).  It does not depend on the cell format
        (an env on 16-bit cells and one on compact cells in the same state have the same key), and never on engine state: the
        layout marker, the episode counter, the generator's words, the running episode.

        env_ids  a contiguous int64 [n] tensor on the env's device (None = every env, in order), read by the kernel as it is; ids
                 may repeat.  An id outside [0, batch) leaves its key as it was and is reported by `check_errors()`.
        salt     any int in [0, 2**64): another salt gives an independent key (two of them: 128 bits)
        out      an int64 [n] tensor on the env's device to write: a caller that keys every step allocates nothing."""
        return row_queries.state_key(self._row_set("state_key"), env_ids, salt, step_count, rng, out)

    def obs_key(self, obs: torch.Tensor | None = None, dir: torch.Tensor | None = None, *, salt: int = 0,
                out: torch.Tensor | None = None) -> torch.Tensor:
        """A 64-bit key per agent observation (include/mgx.h "STATE KEYS": the view's image bytes and its direction; the agent's
        index is no part of it), by ONE launch (mgx_obs_key) on the current stream.  Default: the env's own `obs` / `dir` of the last
        step or gen_obs -> int64 [B, A].  Otherwise any contiguous uint8 [..., v, v, 3] with a matching uint8 [...] on the env's
        device -- a rollout's [T, B, A, ...] outputs -- and the result has the leading shape.  `salt`, `out` as in `state_key()`.  The
        default needs a loaded state and no open persistent session (pass a session's outputs explicitly)."""
        if (obs is None) != (dir is None):
            raise ValueError("obs_key: pass both obs and dir, or neither")
        v, dev = self.spec.view_size, self._cells.device
        if obs is None:                  # (the env's own outputs: there are none before a state is loaded)
            self._need_state()
            obs, dir = self.obs, self.dir
        for name, t in (("obs", obs), ("dir", dir)):
            if not torch.is_tensor(t) or t.dtype is not torch.uint8 or t.device != dev or not t.is_contiguous():
                raise ValueError(f"obs_key: {name} must be a contiguous uint8 tensor on {dev}")
        if obs.dim() < 3 or tuple(obs.shape[-3:]) != (v, v, 3) or tuple(obs.shape[:-3]) != tuple(dir.shape):
            raise ValueError(f"obs_key: obs must have shape [..., {v}, {v}, 3] and dir the leading shape [...], got "
                             f"{tuple(obs.shape)} and {tuple(dir.shape)}")
        _, salt = _key_args("obs_key", salt, False, False)
        keys = _out("obs_key", out, tuple(dir.shape), torch.int64, 0, dev)
        self.join()
        self.backend.obs_key(int(dir.numel()), obs, dir, salt, keys)
        return keys

    def key_table(self, capacity: int):
        """A `multigrid_amd.KeyTable` of `capacity` slots (a power of two, 64 .. 2**30) on the env's device, launched through the
        env's backend: the set of keys already seen -- `state_key()` / `obs_key()` outputs of this env, its snapshots or any other
        int64 numbers -- with a stable entry id per key, visit counts and "which of these are new" (include/mgx.h "KEY TABLES").  The
        table belongs to the caller, not to the env: nothing the env does reads or writes it."""
        from .key_table import KeyTable
        return KeyTable(capacity, self._cells.device, backend=self.backend)

    def selector(self, n_max: int | None = None):
        """A `multigrid_amd.Selector` for up to `n_max` items (None: `batch`) on the env's device, launched through the env's
        backend: the k best of a level by (score, index) as a list of fixed length with the count on the device, and with no scores
        a fixed-shape `nonzero` (include/mgx.h "SELECTION").  It belongs to the caller, not to the env."""
        from .select import Selector
        return Selector(self.batch if n_max is None else n_max, self._cells.device, backend=self.backend)

    # ------------------------------------------------------------------------------------------ action masks
    def action_mask(self, env_ids: torch.Tensor | None = None, *, expand: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
        """Which actions of every agent of the envs `env_ids` can do anything in the state they are in (include/mgx.h "ACTION
        MASKS"): uint8 [n, A] on the device, bit k = `Action` k (left 0 .. toggle 5; `done` and bit 7 are never set), made by ONE
        launch (mgx_action_mask) on the current stream -- no host round trip, no synchronisation, capturable in a graph.  With
        `expand=True` the result is bool [n, A, 7], what `logits.masked_fill(~mask, -inf)` takes.

        A clear bit is a promise: a step in which that agent takes that action and the others `done` equals the step in which it
        takes `done` too -- a search need not fork that child.  A set bit means the step changes the grid or the agent rows (in an
        env with declared hook rules: or may end the episode).  A terminated agent has no bit set; the turns are set for every other
        agent.  The mask does not depend on the cell format and never on engine state.

        env_ids  a contiguous int64 [n] tensor on the env's device (None = every env, in order), read by the kernel as it is; ids
                 may repeat.  An id outside [0, batch) leaves its masks as they were and is reported by `check_errors()`.
        out      a uint8 [n, A] (expand: bool [n, A, 7]) tensor on the env's device to write: a caller that masks every step
                 allocates nothing."""
        return row_queries.action_mask(self._row_set("action_mask"), env_ids, expand, out)

    # ------------------------------------------------------------------------------------------ distance fields
    def distance_field(self, env_ids: torch.Tensor | None = None, *, types=None, colors=None, agents=None, points=None, through=(),
                       avoid_lava: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
        """How many moves every cell of the envs `env_ids` lies from the nearest source cell, walls respected (include/mgx.h
        "DISTANCE FIELDS"): int16 [n, H, W] on the device, -1 for walls, unreachable cells and envs without a source, made by ONE
        launch (mgx_distance) on the current stream -- no host round trip, no synchronisation, capturable in a graph.  Distances
        count moves, not actions: turns are free.  Agents never block; a walk enters what `forward` enters when nobody stands there
        (empty, floor, goal, lava, open doors).  A source need not be passable: the distance to a key is that to the key's cell.

        types       Type members or ints: every cell of such a type is a source ...
        colors      ... if it has one of these Color members or ints (None = any colour; needs types=)
        agents      agent indices: the positions of these agents (terminated or not) are sources
        points      a contiguous int16 [n, P, 2] tensor on the env's device: (x, y) sources per output row; points outside the
                    grid are ignored
        through     a subset of {"closed", "locked", "objects"}: closed doors, locked doors, key / ball / box cells are passable
        avoid_lava  lava is impassable
        env_ids     a contiguous int64 [n] tensor on the env's device (None = every env, in order), read by the kernel as it is;
                    ids may repeat.  An id outside [0, batch) leaves its rows as they were and is reported by `check_errors()`.
        out         an int16 [n, H, W] tensor on the env's device to write: a caller that asks every step allocates nothing.
        Sides above 64 are refused (the kernel holds a grid row in one 64-bit word, an env's rows in one wavefront)."""
        query = dict(types=types, colors=colors, agents=agents, points=points, through=through, avoid_lava=avoid_lava)
        return row_queries.distance(self._row_set("distance_field"), env_ids, query, out, True)

    def agent_distance(self, env_ids: torch.Tensor | None = None, *, types=None, colors=None, agents=None, points=None, through=(),
                       avoid_lava: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
        """The distance field of `distance_field()` -- same arguments, same launch -- read at the agents' positions only: int16
        [n, A], the number of moves from agent a to the nearest source, -1 when there is no way (or the agent row lies outside the
        grid).  A terminated agent is answered like any other.  `out`: an int16 [n, A] tensor to write."""
        query = dict(types=types, colors=colors, agents=agents, points=points, through=through, avoid_lava=avoid_lava)
        return row_queries.distance(self._row_set("agent_distance"), env_ids, query, out, False)

    def outputs_to_host(self) -> dict:
        """Everything the last step / gen_obs handed back, on the host after ONE device-to-host copy (into a pinned buffer) and one
        stream synchronisation: {'reward' f64[B,A], 'obs' u8[B,A,v,v,3], 'dir', 'terminated' u8[B,A], 'truncated' u8[B], 'err'
        i32[2]} as numpy views of that buffer -- valid until the next call.  For host callers of small batches (the dict API steps one
        env: six copies of a few bytes each cost six round trips); a batch's 38 MB of observations belong on the device."""
        self.join()
        if self._out.device.type == "cpu":
            host = self._out
        else:
            if self._out_host is None:
                self._out_host = torch.empty(self._out.shape, dtype=torch.uint8, pin_memory=True)
            self._out_host.copy_(self._out, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            host = self._out_host
        arr = host.numpy()
        out = {}
        for name, dt, shape, off in self._out_parts:
            npdt = {torch.float64: np.float64, torch.uint8: np.uint8, torch.int32: np.int32}[dt]
            n = int(np.prod(shape)) * np.dtype(npdt).itemsize
            out[name] = arr[off:off + n].view(npdt).reshape(shape)
        return out

    def check_errors(self):
        """Synchronises and raises ValueError if any env met an unknown action since the last check -- or, after that, if
        snapshot() / restore() / fork() skipped a pair whose env id or snapshot row was out of range."""
        self.join()
        gb = getattr(self.backend, "_grid_bad", None)
        if gb is not None:                       # byte grids: what the step kernels counted while packing them
            unpackable, ring = (int(v) for v in gb.cpu())
            if unpackable or ring:
                gb.zero_()
                raise ValueError(f"the byte grid held {ring} outer-ring cell(s) that are not WALL = (wall, grey, 0) and {unpackable} "
                                 f"cell value(s) the packed format cannot hold (include/mgx.h)")
        count, first = (int(v) for v in self.err.cpu())
        if count:
            self._reset_err()
            raise ValueError(f"Unknown action in {count} env(s); first at local env {first} "
                             f"(valid: {int(Action.left)}..{int(Action.done)}, or {NO_ACTION} for no action)")
        cb = getattr(self, "_copy_bad", None)
        if cb is not None:                       # snapshot() / restore() / fork(): the pairs the kernel skipped
            count, first = (int(v) for v in cb.cpu())
            if count:
                cb.copy_(torch.tensor([0, INT32_MAX], dtype=torch.int32))
                raise ValueError(f"snapshot / restore / fork: {count} pair(s) named an env id or a snapshot row out of range and "
                                 f"were skipped; first at pair {first}")

    def is_done(self) -> torch.Tensor:
        """multigrid/base.py:534-539 per env: bool[B]."""
        self._no_session("is_done")
        truncated = self.step_count >= self.spec.max_steps
        return truncated | (self.agents[:, :, 4] != 0).all(dim=1)

    def _no_session(self, what: str):
        """The state tensors are stale while a persistent session is open (the state lives in its launch, which writes it back when
        it ends): reading or replacing them then is a mistake, not a race to win."""
        if self._session is not None:
            raise RuntimeError(f"{what}: a persistent session is open -- the env state lives in its launch until it is closed")

    def _need_wide_cells(self, what: str):
        """Device-side generation, anything with env hooks beyond the plain step, one-hot rollouts -- and everything but the plain step
        and gen_obs on byte grids -- are compiled for the 16-bit cells only."""
        if self.spec.compact:
            raise NotImplementedError(f"{what} is not available on compact cells / byte grids (EnvSpec.cell_bytes = 1 or 3: step / "
                                      f"gen_obs / auto-reset from a layout pool / full_obs); build the env with cell_bytes = 2 for it")

    def _need_state(self):
        if not self._loaded:
            raise RuntimeError("no state loaded: call load_state() / reset() first")
        if self._session is not None:
            raise RuntimeError("a persistent session is open: the env state lives in its launch until it is closed")

    def persistent(self, max_steps: int, auto_reset: bool = False, timeout_ms: int = 2000) -> "PersistentSession":
        """A `PersistentSession` over this env: closed-loop stepping with ONE resident launch instead of one launch per step
        (include/mgx.h: mgx_step_persistent).  Same results as `step()` bit for bit.  `max_steps` bounds the launch; every wait
        inside it gives up after `timeout_ms`."""
        if self._stats is not None:
            raise RuntimeError("episode accounting (track_episodes) does not follow persistent stepping: the env state lives in the "
                               "resident launch; track_episodes(None) first")
        if not (self.spec.cell_bytes == 1 and self.spec.env_kind == "empty"):
            self._need_wide_cells("persistent stepping")                    # (compact cells: the hook-free persistent launch, round 6)
        return PersistentSession(self, max_steps, auto_reset, timeout_ms)

    # ------------------------------------------------------------------------------------------ checkpoint
    def state_dict(self) -> dict:
        """Everything a resumed run needs to continue bit-identically: the env state, and -- when auto-reset is in use --
        the layout pool, the per-env episode counters and the last `was_reset`."""
        self._no_session("state_dict")
        self.join()
        sd = {"spec": self.spec.as_dict(), "first_env": self.first_env,
              "grid": self.grid.cpu().clone(), "agents": self.agents.cpu().clone(),
              "rng": self.rng.cpu().clone(), "step_count": self.step_count.cpu().clone(),
              "aux": self.aux.cpu().clone()}
        if getattr(self, "_gen", None) is not None:
            sd["generator"] = {"kind": self._gen["kind"], "room_size": self._gen["room_size"], "start": self._gen["start"],
                               "max_hallway_keys": self._gen["max_hallway_keys"], "max_keys_per_room": self._gen["max_keys_per_room"],
                               "gen_state": self._gen["gen_state"].cpu().clone()}
            sd["episode"] = self.episode.cpu().clone()
            sd["was_reset"] = self.was_reset.cpu().clone()
        if getattr(self, "_pool", None) is not None:
            pg, pa, pt = self._pool
            sd["pool"] = {"grid": torch.from_numpy(layouts.unpack_cells_for(self.spec, pg.cpu().numpy())), "agents": pa.cpu().clone(),
                          "aux": pt.cpu().clone() if pt is not None else None}
            sd["episode"] = self.episode.cpu().clone()
            sd["was_reset"] = self.was_reset.cpu().clone()
        return sd

    def load_state_dict(self, sd: dict):
        self._no_session("load_state_dict")
        if EnvSpec.from_dict(sd["spec"]) != self.spec:
            raise ValueError("state_dict was saved for a different EnvSpec")
        if int(sd.get("first_env", self.first_env)) != self.first_env:
            raise ValueError(f"state_dict was saved for the shard starting at env {sd['first_env']}, this one starts "
                             f"at {self.first_env} (layout choice and seeds are functions of the global env index)")
        self.load_state(sd["grid"], sd["agents"], sd["rng"], sd["aux"], sd["step_count"], validate=True)
        if sd.get("generator") is not None:
            g = sd["generator"]
            self.set_layout_generator(g["kind"], 0, room_size=g["room_size"], start=g["start"],
                                      max_hallway_keys=g.get("max_hallway_keys", 1), max_keys_per_room=g.get("max_keys_per_room", 2))
            self._gen["gen_state"].copy_(g["gen_state"])
            self.episode.copy_(sd["episode"])
            self.was_reset.copy_(sd["was_reset"])
        if sd.get("pool") is not None:
            p = sd["pool"]
            self.set_layout_pool(p["grid"].numpy(), p["agents"].numpy(), p["aux"].numpy() if p["aux"] is not None else None)
            self.episode.copy_(sd["episode"])
            self.was_reset.copy_(sd["was_reset"])
