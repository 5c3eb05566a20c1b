"""The sizes at which a step with auto-reset READS the layout marker (include/mgx.h: mgx_step_tracked), and what the tests of
tests/test_marker_sizes_gpu.py and tests/test_jit_forms_gpu.py share.  No tests in here, and nothing that needs a GPU.

  * `reads_marker(spec, B, pool_size)`: a Python mirror of the rule by which a launch reads the marker, written from include/mgx.h
    and the comment above plan_marker_read (csrc/mgx_kernels.hip) -- the library is asked for the launch geometry only;
  * `smallest_reading_batch(spec)`: the least batch of more than 2048 wavefronts; `SIZES`: one case per grid size that qualifies;
  * `oracle_run(name)`: T steps with auto-reset of a SAMPLE of whole wavefronts on the oracle backend (the first two, two in the
    middle, the last two -- the last one partial), with a model of the marker beside them and the census of what the run met.  The
    census comes from the oracle alone: the kernel under test cannot satisfy it by being wrong."""
import functools

import numpy as np
import torch

from multigrid_amd import EnvSpec, _lib, layouts
from oracle import binding as ob
from tests import util
from tests.test_grid_layout_marker import make_env

T_STEPS = 12
PICKUP, DROP, TOGGLE, DONE = 3, 4, 5, 6
OUT = ("obs", "dir", "reward", "terminated", "truncated", "was_reset")
STATE = ("_cells", "agents", "rng", "step_count", "aux", "episode")
CENSUS = ("wavefront_all_marked", "wavefront_mixed", "marked_env_dirtied", "unmarked_env_restarted")


def wavefronts(spec, B) -> int:
    return -(-B // _lib.launch_info(spec, B)["envs_per_wavefront"])


def smallest_reading_batch(spec) -> int:
    """The least B whose plain step has more than 2048 wavefronts.  The envs per wavefront depend on B (small batches get fewer), so
    the candidate 2048 G + 1 is tried for every G the spec is ever given, smallest first."""
    seen, B = set(), 1
    while True:                                              # every envs-per-wavefront value the library chooses for this spec
        G = _lib.launch_info(spec, B)["envs_per_wavefront"]
        if G in seen:
            break
        seen.add(G)
        B = 2048 * G + 1
    for G in sorted(seen):
        B = 2048 * G + 1
        if wavefronts(spec, B) > 2048:
            assert wavefronts(spec, B - 1) <= 2048
            return B
    raise AssertionError(f"{spec}: no batch of more than 2048 wavefronts found")


def throughput_batch_of_2048_wavefronts(spec):
    """A batch of EXACTLY 2048 wavefronts that is nevertheless stepped by the throughput family (more than 32 view slots per
    wavefront: no latency instantiation), or None: the launch at which `> 2048` and `>= 2048` differ."""
    from multigrid_amd import jit
    for G in (1, 2, 4, 8, 16, 32, 64):
        B = 2048 * G
        if wavefronts(spec, B) == 2048 and not jit.shape_key(spec, B).dma:
            return B
    return None


def reads_marker(spec, B, pool_size, pool_aligned=True) -> bool:
    """include/mgx.h (mgx_step_tracked): "launches of the throughput family (more than 2048 wavefronts) with a one-layout pool also
    READ it ... grids of a power-of-two size up to 1 KiB", 16-bit cells; the comment above plan_marker_read adds the bounds: at least
    one 16-byte vector per grid, a wavefront's tile of at most one 8 KiB burst, a 16-byte aligned pool."""
    G = _lib.launch_info(spec, B)["envs_per_wavefront"]
    grid_bytes = spec.width * spec.height * 2
    return (spec.cell_bytes == 2 and -(-B // G) > 2048 and pool_size == 1 and 16 <= grid_bytes <= 1024
            and grid_bytes & (grid_bytes - 1) == 0 and G * grid_bytes <= 8192 and pool_aligned)


# ---- the sizes ----------------------------------------------------------------------------------------------------------------------

#: name -> (spec, seed of the layout, envs in the last wavefront).  W, H, A, view as the grid sizes between 32 bytes and 1 KiB ask.
SIZES = {
    "4x4_a1_v3": (EnvSpec(4, 4, 1, 3, max_steps=4), 0, 1),                        # 32 bytes; A == 1; a lone env in the last wavefront
    "8x4_a2_v3": (EnvSpec(8, 4, 2, 3, max_steps=4), 9, 3),                        # 64
    "8x8_a2_v7": (EnvSpec(8, 8, 2, 7, max_steps=5), 6, 5),                        # 128
    "rbd16x8_a2_v7": (EnvSpec(16, 8, 2, 7, max_steps=5, env_kind="redbluedoors"), 6, 7),     # 256, hooks and pool_aux
    "8x16_a3_v5": (EnvSpec(8, 16, 3, 5, max_steps=5), 7, 2),                      # 256, the other orientation, A no power of two
    "32x16_a2_v7": (EnvSpec(32, 16, 2, 7, max_steps=5), 8, 1),                    # 1024: the upper bound; a lone env again
}
#: the size whose throughput kernel tests/test_jit_forms_gpu.py compiles at run time and registers.  A registration lasts for the
#: process and serves every env of its geometry: a view size of its own keeps the 8x8 case above on the library's kernel
JIT_SIZES = {"8x8_a2_v5_jit": (EnvSpec(8, 8, 2, 5, max_steps=5), 6, 5)}
CASES = dict(SIZES, **JIT_SIZES)
# (the seeds: of 1 .. 12, one per size whose ORACLE run meets every condition of the census and ends episodes by termination too;
# max_steps <= 5, so that an env that starts at step 0 restarts twice within the 12 steps by truncation alone)


def batch_of(name) -> int:
    spec, _, tail = CASES[name]
    B0 = smallest_reading_batch(spec)                        # (its last wavefront holds one env)
    B = B0 + tail - 1
    G = _lib.launch_info(spec, B)["envs_per_wavefront"]
    assert wavefronts(spec, B) == 2049 and B % G == tail and tail < G, (name, B, G)
    return B


def pool_for(spec, seed):
    """ONE layout: (grids u8[1,H,W,3], agents u8[1,A,8], auxs u8[1,16] | None)"""
    W, H, A = spec.width, spec.height, spec.num_agents
    if W * H <= 16:
        # 2 x 2 free cells: random placement at density 0.3 leaves nothing to act on.  The Empty layout and one object: the agent at
        # (1, 1) faces a key; the goal in the far corner
        g = np.zeros((H, W, 3), np.uint8)
        g[...] = (2, 5, 0)
        g[1:H - 1, 1:W - 1] = (1, 0, 0)
        g[H - 2, W - 2] = (8, 1, 0)
        g[1, 2] = (5, 4, 0)
        a = np.zeros((A, 8), np.uint8)
        a[:, 0] = np.arange(A) % 6
        a[:, 2:4] = 1
        a[:, 5] = 1
        return g[None], a[None], None
    st = util.random_state(spec, 1, seed, density=0.3, terminated_p=0.0)
    g, a, x = st["grid"], st["agents"], None
    if spec.env_kind == "redbluedoors":
        # the two doors the hook watches, closed, a quarter of the width from either side (multigrid/envs/redbluedoors.py:158-168)
        ry, by = 1 + seed % (H - 2), 1 + (seed + 3) % (H - 2)
        rx, bx = W // 4, W // 4 + W // 2 - 1
        taken = {(int(r[2]), int(r[3])) for r in a[0]}
        assert (rx, ry) not in taken and (bx, by) not in taken, "an agent stands where a door goes: another seed"
        g[0, ry, rx] = (4, 0, 1)
        g[0, by, bx] = (4, 2, 1)
        x = np.zeros((1, 16), np.uint8)
        x[0, :4] = (bx, by, rx, ry)
    return g, a, x


def sample_of(spec, B):
    """Whole wavefronts as (lo, hi) env ranges: the first two, two in the middle, the last two (the last one partial)"""
    G = _lib.launch_info(spec, B)["envs_per_wavefront"]
    nw = -(-B // G)
    return [(w * G, min((w + 1) * G, B)) for w in sorted({0, 1, nw // 2, nw // 2 + 1, nw - 2, nw - 1})]


def host_actions(T, B, A, seed):
    """i8[T,B,A]: uniform over the seven actions, every fourth one replaced by pickup / toggle / drop in turn"""
    r = np.random.default_rng([seed, B, A])
    a = r.integers(0, 7, size=(T, B, A)).astype(np.int8)
    hit = r.random((T, B, A)) < 0.25
    a[hit] = np.array([PICKUP, TOGGLE, DROP], np.int8)[r.integers(0, 3, size=int(hit.sum()))]
    return a


class Run:
    """What `oracle_run` keeps: per step and sampled wavefront the outputs, the state and the marker's model"""

    def __init__(self, spec, B, pool, sample, acts):
        self.spec, self.B, self.pool, self.sample, self.acts = spec, B, pool, sample, acts
        self.idx = np.concatenate([np.arange(lo, hi) for lo, hi in sample])
        self.steps, self.census, self.ambiguous = [], dict.fromkeys(CENSUS, 0), []


def model_marker(m, start_cells, cells, start_carry, rows, was_reset, acts):
    """include/mgx.h: "a restart from the pool stores the layout's index, every cell written back to `grid` stores -1".  `m`: i32[n]
    before the step, updated in place.  Returns (dirtied, ambiguous): the envs whose grid the step changed, and those whose grid
    is as it was although two agents' hands changed (a drop and a pickup) or two agents toggled: one may have undone the other's
    write within the step.  The final grids cannot tell, and there the kernel's -1 is as right as the model's value.  (One agent
    alone cannot write a cell and leave the grid as it was: every pickup, drop and toggle that succeeds changes its cell.)"""
    m[was_reset != 0] = 0
    dirtied = (cells != start_cells).reshape(len(m), -1).any(axis=1)
    m[dirtied] = -1
    hands = (rows[:, :, 5:8] != start_carry).any(axis=2).sum(axis=1) >= 2
    # two agents that toggle the SAME cell (a toggle moves nobody: the rows after the step name the cell in front)
    d = rows[:, :, 1].astype(np.int64)
    fx = rows[:, :, 2].astype(np.int64) + np.array([1, 0, -1, 0])[d]
    fy = rows[:, :, 3].astype(np.int64) + np.array([0, 1, 0, -1])[d]
    front = np.where(acts == TOGGLE, fy * 256 + fx, -1 - np.arange(acts.shape[1])[None])
    front = np.sort(front, axis=1)
    toggles = (front[:, 1:] == front[:, :-1]).any(axis=1) if acts.shape[1] > 1 else np.zeros(len(m), bool)
    return dirtied, (hands | toggles) & ~dirtied & (m >= 0)


def run_oracle(spec, B, pool, sample, acts, seed=3) -> Run:
    run = Run(spec, B, pool, sample, acts)
    envs = [make_env(spec, B, pool, device="cpu", backend=util.OracleBackend(spec, nthreads=4), seed=seed, rows=r) for r in sample]
    layout = layouts.pack_cells_for(spec, pool[0])[0].view(np.int16)
    marks = [np.where((e._cells.numpy() == layout).reshape(e.batch, -1).all(axis=1), 0, -1).astype(np.int32) for e in envs]
    for t in range(acts.shape[0]):
        rec = {k: [] for k in OUT + STATE + ("_marker", "ambiguous")}
        for e, (lo, hi), m in zip(envs, sample, marks):
            before, hands = e._cells.numpy().copy(), e.agents.numpy()[:, :, 5:8].copy()
            m0 = m.copy()
            e.step(torch.from_numpy(acts[t, lo:hi]), auto_reset=True)
            wr = e.was_reset.numpy()
            start = np.where(wr.astype(bool)[:, None, None], layout[None], before)
            start_hands = np.where(wr.astype(bool)[:, None, None], pool[1][:, :, 5:8], hands)
            dirtied, amb = model_marker(m, start, e._cells.numpy(), start_hands, e.agents.numpy(), wr, acts[t, lo:hi])
            c = run.census
            c["wavefront_all_marked"] += int((m0 == 0).all())
            c["wavefront_mixed"] += int((m0 == 0).any() and (m0 < 0).any())
            c["marked_env_dirtied"] += int((dirtied & ((m0 == 0) | (wr != 0))).sum())
            c["unmarked_env_restarted"] += int(((m0 < 0) & (wr != 0)).sum())
            for k in OUT + STATE:
                rec[k].append(getattr(e, k).numpy().copy())
            rec["_marker"].append(m.copy())
            rec["ambiguous"].append(amb)
            e.check_errors()
        run.steps.append({k: np.concatenate(v) for k, v in rec.items()})
    assert min(int(e.episode.min()) for e in envs) >= 2, "an env of the sample restarted fewer than two times"
    return run


@functools.lru_cache(maxsize=None)
def oracle_run(name) -> Run:
    spec, seed, _ = CASES[name]
    B = batch_of(name)
    return run_oracle(spec, B, pool_for(spec, seed), sample_of(spec, B), host_actions(T_STEPS, B, spec.num_agents, seed))


def visible_change(spec, pool):
    """The layout with one cell replaced so that the agents' observations differ (by the oracle): (grid u8[H,W,3], (y, x))"""
    g, a = pool[0][0], pool[1][0]
    d = spec.as_dict()
    want = ob.gen_obs_batch(d, g[None].copy(), a[None].copy(), 1)[0]
    under = {(int(r[3]), int(r[2])) for r in a}
    for y in range(1, spec.height - 1):
        for x in range(1, spec.width - 1):
            if (y, x) in under:
                continue
            other = g.copy()
            other[y, x] = (6, 2, 0) if tuple(g[y, x]) != (6, 2, 0) else (5, 1, 0)
            if ob.gen_obs_batch(d, other[None].copy(), a[None].copy(), 1)[0].tobytes() != want.tobytes():
                return other, (y, x)
    raise AssertionError("no cell of the layout is seen by an agent")
