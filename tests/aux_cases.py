"""The GPU cases of the streaming kernels in csrc/mgx_aux.hip (one_hot, full_obs, pack / unpack / check_grid, reset_done), their random
inputs and their plain NumPy references, written from the words of include/mgx.h.

Each of those kernels picks between fast and slow paths by pointer alignment, by a group size the launcher derives from the batch and by
tail length.  A case names the branches it is meant to reach (`labels`); tests/test_aux_branch_census.py derives on the CPU, from the
launchers' own arithmetic (csrc/mgx_aux_geom.h through tests/hostshim), which branches each case DOES reach and fails when the two
part: the fix is then to this table.  tests/test_aux_kernels_gpu.py runs the cases.
"""
import collections
import zlib

import numpy as np

T_WALL, T_DOOR, T_BOX, T_AGENT = 2, 4, 7, 10
WALL3 = (2, 5, 0)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ===================================================================================================================== cells
def valid_triples(r, shape, compact=False, content_p=0.5):
    """Random VALID (type, color, state) bytes u8[shape + (3,)]: every type the reference has (0..10), colours 0..5, states 0..2 (a
    direction 0..3 on an agent overlay); `compact`: what one byte can hold -- a state only on doors and agent overlays, no box content.
    Otherwise boxes hold things with probability `content_p` (state byte | kind << 2 | colour << 5, include/mgx.h "BOX CONTENTS")."""
    t = r.integers(0, 11, size=shape, dtype=np.uint8)
    c = r.integers(0, 6, size=shape, dtype=np.uint8)
    s = r.integers(0, 3, size=shape, dtype=np.uint8)
    s = np.where(t == T_AGENT, r.integers(0, 4, size=shape, dtype=np.uint8), s)
    if compact:
        s = np.where((t == T_DOOR) | (t == T_AGENT), s, 0).astype(np.uint8)
    else:
        kind = r.integers(1, 8, size=shape, dtype=np.uint8)
        ccol = r.integers(0, 6, size=shape, dtype=np.uint8)
        filled = (t == T_BOX) & (r.random(size=shape) < content_p)
        s = np.where(filled, s | (kind << 2) | (ccol << 5), s).astype(np.uint8)
    return np.stack((t, c, s), axis=-1)


def valid16(g):
    """include/mgx.h: what the 16-bit packed format can hold -- type <= 15, color <= 7, state <= 3; a state byte above 3 is a BOX's content
    (kind 1..7, colour <= 5)."""
    t, c, sb = g[..., 0], g[..., 1], g[..., 2]
    kind, ccol = (sb >> 2) & 7, sb >> 5
    return (t <= 15) & (c <= 7) & (((sb >> 2) == 0) | ((t == T_BOX) & (kind != 0) & (ccol <= 5)))


def valid8(g):
    """... and the compact format: additionally no box content, a state only on a door (1, 2) or an agent overlay (1..3), and none of the
    types 11..15 (they are the joint codes of those)."""
    t, sb = g[..., 0], g[..., 2]
    return valid16(g) & ((sb >> 2) == 0) & (t <= 10) & ((sb == 0) | ((t == T_DOOR) & (sb <= 2)) | (t == T_AGENT))


def ring_mask(H, W):
    m = np.zeros((H, W), bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return m


# ===================================================================================================================== full_obs
FullObsCase = collections.namedtuple("FullObsCase", "W H cb B A G labels")
#: (labels: see tests/test_aux_branch_census.py: full_obs_reached)
FULL_OBS = [
    FullObsCase(5, 5, 2, 12289, 3, 3, ("G>1", "cell_bytes 2", "group crosses env", "output-ordered", "input-ordered", "<=3 leftover cells",
                                        "non-pow2", "single loop", "input-ordered single loop")),
    FullObsCase(5, 5, 1, 24577, 2, 6, ("G>1", "cell_bytes 1", "group crosses env", "output-ordered", "input-ordered", "non-pow2", "ragged last wave")),
    FullObsCase(5, 5, 3, 49153, 4, 11, ("G>1", "cell_bytes 3", "group crosses env", "output-ordered", "input-ordered", "<=3 leftover cells",
                                         "eight-in-flight loop", "input-ordered four-in-flight loop", "ragged last wave")),
    FullObsCase(5, 5, 2, 331700, 2, 81, ("G>1", "group crosses env", "output-ordered", "input-ordered", "eight-in-flight loop", "single loop",
                                          "input-ordered four-in-flight loop", "ragged last wave")),
    FullObsCase(3, 3, 2, 929797, 3, 227, ("G>1", "G max", "group crosses env", "output-ordered", "input-ordered", "ragged last wave")),
    FullObsCase(3, 5, 1, 131073, 4, 17, ("G>1", "cell_bytes 1", "group crosses env", "output-ordered", "input-ordered", "ragged last wave")),
    FullObsCase(9, 7, 2, 16386, 5, 4, ("G>1", "group crosses env", "output-ordered", "non-pow2", "ragged last wave")),
    FullObsCase(7, 5, 2, 32771, 2, 8, ("G>1", "group crosses env", "output-ordered", "eight-in-flight loop", "ragged last wave")),
    FullObsCase(4, 8, 2, 65539, 3, 16, ("G>1", "pow2", "output-ordered", "eight-in-flight loop", "ragged last wave")),
    FullObsCase(8, 4, 2, 262143, 2, 64, ("G>1", "pow2", "output-ordered", "eight-in-flight loop", "ragged last wave")),
    FullObsCase(16, 16, 2, 32769, 4, 8, ("G>1", "pow2", "output-ordered", "eight-in-flight loop", "ragged last wave")),      # the bench's form
]
FULL_OBS_IDS = [f"{c.W}x{c.H}_cb{c.cb}_B{c.B}_G{c.G}" for c in FULL_OBS]
ORACLE_ENVS = 64


def full_obs_inputs(case):
    """(cells as the device holds them -- u8[B,H,W] / u16[B,H,W] / u8[B,H,W,3] --, the (type, color, state) bytes they were made from,
    agents u8[B,A,8]).  Every cell of the grid is random (the kernel needs no wall ring); boxes hold things (cell_bytes 2, 3); agents
    stand anywhere, stacked heavily; about 3 % of the rows are out of range (x >= W or y >= H)."""
    from multigrid_amd import layouts
    W, H, cb, B, A = case.W, case.H, case.cb, case.B, case.A
    r = _rng("full_obs", W, H, cb, B)
    g3 = valid_triples(r, (B, H, W), compact=cb == 1)
    cells = layouts.pack_cells8(g3) if cb == 1 else (layouts.pack_cells(g3) if cb == 2 else g3)
    ag = np.zeros((B, A, 8), np.uint8)
    ag[..., 0] = r.integers(0, 6, size=(B, A))
    ag[..., 1] = r.integers(0, 4, size=(B, A))
    ag[..., 2] = r.integers(0, W, size=(B, A))
    ag[..., 3] = r.integers(0, H, size=(B, A))
    stack = r.random(size=(B, A)) < 0.5                                   # ... on agent 0's cell
    ag[..., 2] = np.where(stack, ag[:, :1, 2], ag[..., 2])
    ag[..., 3] = np.where(stack, ag[:, :1, 3], ag[..., 3])
    out = r.random(size=(B, A))
    ag[..., 2] = np.where(out < 0.015, r.integers(W, 256, size=(B, A)), ag[..., 2])
    ag[..., 3] = np.where((out >= 0.015) & (out < 0.03), r.integers(H, 256, size=(B, A)), ag[..., 3])
    ag[..., 4] = r.integers(0, 2, size=(B, A))                            # terminated or not: drawn all the same
    ag[..., 5:8] = valid_triples(r, (B, A), compact=cb == 1)
    return np.ascontiguousarray(cells), g3, ag


def full_obs_reference(g3, agents):
    """include/mgx.h: out u8[B, W, H, 3] = Grid.state ([x][y]) -- a box shown as (box, color, state) whatever it holds -- with every agent's
    (10, color, dir) written at its position in index order; a row with x >= W or y >= H writes nothing."""
    B, H, W, _ = g3.shape
    out = np.ascontiguousarray(g3.transpose(0, 2, 1, 3)).copy()
    out[..., 2] &= 3                                                       # (the content rides in the state byte's upper bits)
    env = np.arange(B)
    for a in range(agents.shape[1]):
        x, y = agents[:, a, 2].astype(np.int64), agents[:, a, 3].astype(np.int64)
        ok = (x < W) & (y < H)
        cell = np.stack((np.full(B, T_AGENT, np.uint8), agents[:, a, 0], agents[:, a, 1]), axis=-1)
        out[env[ok], x[ok], y[ok]] = cell[ok]
    return out


# ===================================================================================================================== one_hot
ONE_HOT_D = (3, 4, 15, 16, 17, 21, 31, 32)
ONE_HOT_N = (1, 4, 5, 1019, 1020, 1021, 1022, 1023, 1024, 1025, 2047, 2048, 2049)
ONE_HOT_BIG = (4096 * 1024 + 1024 + 5, (1, 1, 1))
#: the dims the whole sweep of n and of input offsets runs on: the reference's, D = 3, bit 31 in each field
ONE_HOT_SWEEP_DIMS = ((11, 6, 4), (1, 1, 1), (30, 1, 1), (1, 30, 1), (1, 1, 30), (10, 11, 11), (5, 6, 6))


def one_hot_dims():
    """every (d0, d1, d2) >= 1 with d0 + d1 + d2 in ONE_HOT_D"""
    return [(d0, d1, D - d0 - d1) for D in ONE_HOT_D for d0 in range(1, D - 1) for d1 in range(1, D - d0)]


def one_hot_reference(cells, dims):
    """include/mgx.h: out[c, off_d + cells[c, d]] = 1, everything else 0; a value >= dim_sizes[d] sets no channel of field d."""
    n = cells.shape[0]
    out = np.zeros((n, sum(dims)), np.uint8)
    off, idx = 0, np.arange(n)
    for k, d in enumerate(dims):
        ok = cells[:, k] < d
        out[idx[ok], off + cells[ok, k].astype(np.int64)] = 1
        off += d
    return out


# ===================================================================================================================== pack / unpack
PACK_N = (1, 7, 8, 9, 2047, 2048, 2049)
#: (W, H, B): grids so small that one thread's 8 cells span rows and envs, ragged totals over more than one workgroup, one ordinary size
PACK_ENV = ((3, 3, 1), (3, 3, 229), (3, 4, 171), (5, 3, 137), (9, 7, 33), (16, 16, 9))


def pack_cells3(r, shape, compact=False):
    """(type, color, state) bytes, half of them valid cells (what the packed value is compared on), half drawn from all 256^3 values
    (uniform bytes alone would leave about one valid cell in a thousand)."""
    g = valid_triples(r, shape, compact=compact)
    wild = r.integers(0, 256, size=tuple(shape) + (3,), dtype=np.uint8)
    return np.where((r.random(size=shape) < 0.5)[..., None], g, wild)


def pack_env_cells3(r, B, H, W, compact=False):
    """... as whole env grids: the ring is WALL but for about one cell in ten"""
    g = pack_cells3(r, (B, H, W), compact)
    keep = ring_mask(H, W)[None] & (r.random(size=(B, H, W)) < 0.9)
    g[keep] = WALL3
    return g


def ring_bad(g3):
    """bad[1]: cells of an env's outer ring that are not the reference's WALL = (wall, grey, 0)"""
    B, H, W, _ = g3.shape
    return int((ring_mask(H, W)[None] & (g3 != np.array(WALL3, np.uint8)).any(-1)).sum())


# ===================================================================================================================== check_grid
CheckCase = collections.namedtuple("CheckCase", "W H A B cb")
CHECK = [CheckCase(9, 7, 3, 300, 2), CheckCase(9, 7, 3, 300, 1), CheckCase(3, 3, 32, 100, 2), CheckCase(3, 3, 32, 100, 1),
         CheckCase(3, 3, 1, 1001, 2), CheckCase(5, 3, 2, 411, 1), CheckCase(16, 16, 4, 137, 2)]
CHECK_IDS = [f"{c.W}x{c.H}_a{c.A}_B{c.B}_cb{c.cb}" for c in CHECK]
CELL_CLASSES16 = ("content bits", "type", "colour", "state", "opaque bit")
CELL_CLASSES8 = ("colour", "opaque bit")
AGENT_CLASSES = ("x", "y", "dir", "terminated", "colour", "carry type", "carry colour", "carry state", "carry content")


def valid_state(r, W, H, A, B, cb):
    """(packed cells u16 / u8 [B,H,W], agents u8[B,A,8]) without any violation"""
    from multigrid_amd import layouts
    g3 = valid_triples(r, (B, H, W), compact=cb == 1)
    g3[:, ring_mask(H, W)] = WALL3
    if cb != 1:
        g3[..., 2] = np.where(g3[..., 0] == T_AGENT, g3[..., 2] % 3, g3[..., 2])      # (state 3 exists only as the compact overlay's direction)
    cells = layouts.pack_cells8(g3) if cb == 1 else layouts.pack_cells(g3)
    ag = np.zeros((B, A, 8), np.uint8)
    ag[..., 0] = r.integers(0, 6, size=(B, A))
    ag[..., 1] = r.integers(0, 4, size=(B, A))
    ag[..., 2] = r.integers(1, W - 1, size=(B, A))
    ag[..., 3] = r.integers(1, H - 1, size=(B, A))
    ag[..., 4] = r.integers(0, 2, size=(B, A))
    ag[..., 5:8] = valid_triples(r, (B, A), compact=cb == 1)
    ag[..., 7] = np.where(ag[..., 5] == T_AGENT, ag[..., 7] % 3, ag[..., 7])
    return cells, ag


def check_inputs(case):
    """A valid state with DENSE random defects: one cell in eight is a uniformly random bit pattern, one ring cell in ten a random valid
    cell, and each field of an agent row is a random byte with probability 1/10."""
    W, H, A, B, cb = case
    r = _rng("check", *case)
    cells, ag = valid_state(r, W, H, A, B, cb)
    wild = r.integers(0, 1 << (8 * cb), size=cells.shape).astype(cells.dtype)
    cells = np.where(r.random(size=cells.shape) < 0.125, wild, cells)
    rand = r.integers(0, 256, size=ag.shape, dtype=np.uint8)
    ag = np.where(r.random(size=ag.shape) < 0.1, rand, ag)
    return np.ascontiguousarray(cells), np.ascontiguousarray(ag)


def cell_defects(cells, cb):
    """per class of include/mgx.h (mgx_check_grid, bad[0]): the cells that show it"""
    p = cells.astype(np.uint32)
    if cb == 1:
        tc, col, opaque = p & 15, (p >> 4) & 7, (p >> 7) & 1
        want = (tc == T_WALL) | (tc == 11) | (tc == 12)                   # a wall, a door that is not open
        return {"colour": col > 5, "opaque bit": opaque != want}
    t, col, st, opaque = p & 15, (p >> 8) & 7, (p >> 12) & 3, (p >> 15) & 1
    kind, ccol = (p >> 4) & 7, ((p >> 7) & 1) | (((p >> 11) & 1) << 1) | (((p >> 14) & 1) << 2)
    want = (t == T_WALL) | ((t == T_DOOR) & (st != 0))
    return {"content bits": ((kind | ccol) != 0) & ((t != T_BOX) | (kind == 0) | (ccol > 5)),
            "type": t > 10, "colour": col > 5, "state": st > 2, "opaque bit": opaque != want}


def agent_defects(ag, W, H, cb):
    """... and of an agent row (bad[2])"""
    x, y, cs = ag[..., 2].astype(int), ag[..., 3].astype(int), ag[..., 7]
    kind, ccol = (cs >> 2) & 7, cs >> 5
    return {"x": (x < 1) | (x > W - 2), "y": (y < 1) | (y > H - 2), "dir": ag[..., 1] > 3, "terminated": ag[..., 4] > 1,
            "colour": ag[..., 0] > 5, "carry type": ag[..., 5] > 10, "carry colour": ag[..., 6] > 5, "carry state": (cs & 3) > 2,
            "carry content": ((cs >> 2) != 0) & ((cb == 1) | (ag[..., 5] != T_BOX) | (kind == 0) | (ccol > 5))}


def check_reference(cells, ag, W, H, cb):
    """the four words of mgx_check_grid from include/mgx.h; `ag` may be None"""
    B = cells.shape[0]
    fmt = np.zeros(cells.shape, bool)
    for m in cell_defects(cells, cb).values():
        fmt |= m
    ring = ring_mask(H, W)[None] & (cells != (0xD2 if cb == 1 else 0x8502))
    env_bad = fmt.any((1, 2)) | ring.any((1, 2))
    nag = 0
    if ag is not None:
        abad = np.zeros(ag.shape[:2], bool)
        for m in agent_defects(ag, W, H, cb).values():
            abad |= m
        nag = int(abad.sum())
        env_bad |= abad.any(1)
    first = int(np.argmax(env_bad)) if env_bad.any() else 2 ** 31 - 1
    return [int(fmt.sum()), int(ring.sum()), nag, first]


# ===================================================================================================================== reset_done
#: W, H, cb, A, K, B, pool base offset in bytes, aux, first_env; (unit, units >= 64) is what the launcher is to choose
ResetCase = collections.namedtuple("ResetCase", "W H cb A K B pool_off aux first_env unit big")
FAR = 2 ** 40 + 5
RESET = [
    ResetCase(4, 4, 2, 3, 7, 333, 0, False, FAR, 16, False),
    ResetCase(32, 16, 2, 4, 7, 300, 0, False, 3, 16, True),
    ResetCase(4, 4, 1, 3, 7, 333, 0, False, FAR, 16, False),            # (ONE unit per env: the division by `units` is by one)
    ResetCase(6, 6, 2, 1, 7, 333, 0, True, FAR, 8, False),
    ResetCase(26, 20, 1, 3, 1, 300, 0, False, 0, 8, True),
    ResetCase(5, 6, 2, 4, 7, 333, 0, False, 11, 4, False),
    ResetCase(10, 13, 2, 1, 7, 300, 0, False, FAR, 4, True),
    ResetCase(3, 3, 2, 3, 7, 333, 0, False, FAR, 2, False),
    ResetCase(5, 13, 2, 4, 1, 300, 0, False, 5, 2, True),
    ResetCase(3, 3, 1, 1, 7, 333, 0, False, 0, 1, False),
    ResetCase(3, 3, 3, 3, 7, 333, 0, False, FAR, 1, False),
    ResetCase(9, 9, 1, 4, 7, 300, 0, False, 9, 1, True),
    # a pool whose base is offset: the 32-byte layout of a 4x4 grid is copied in units of 8 and of 2 bytes
    ResetCase(4, 4, 2, 3, 7, 333, 8, False, FAR, 8, False),
    ResetCase(4, 4, 2, 4, 7, 333, 2, False, 1, 2, False),
    ResetCase(16, 16, 2, 3, 7, 300, 4, False, 2, 4, True),
]
RESET_IDS = [f"{c.W}x{c.H}_cb{c.cb}_a{c.A}_K{c.K}_off{c.pool_off}_unit{c.unit}{'_big' if c.big else ''}" for c in RESET]
RESET_MAX_STEPS = 50


def reset_inputs(case):
    """Random env and pool state; about 40 % of the envs are finished (half of those by all agents terminated, half by step_count)."""
    W, H, cb, A, K, B = case[:6]
    r = _rng("reset", *case)
    shape = (H, W, 3) if cb == 3 else (H, W)
    dt = np.uint16 if cb == 2 else np.uint8
    hi = 1 << (16 if cb == 2 else 8)
    st = dict(grid=r.integers(0, hi, size=(B,) + shape).astype(dt), pool_grid=r.integers(0, hi, size=(K,) + shape).astype(dt),
              agents=r.integers(0, 256, size=(B, A, 8), dtype=np.uint8), pool_agents=r.integers(0, 256, size=(K, A, 8), dtype=np.uint8),
              aux=r.integers(0, 256, size=(B, 16), dtype=np.uint8), pool_aux=r.integers(0, 256, size=(K, 16), dtype=np.uint8),
              episode=r.integers(0, 1000, size=B).astype(np.int32), step_count=r.integers(0, RESET_MAX_STEPS, size=B).astype(np.int32))
    how = r.random(size=B)
    st["agents"][..., 4] = r.integers(0, 2, size=(B, A))
    st["agents"][:, 0, 4] = 0                                              # somebody still acts ...
    st["agents"][how < 0.2, :, 4] = r.integers(1, 256, size=(int((how < 0.2).sum()), A))      # ... but where all are terminated (any non-zero byte)
    late = (how >= 0.2) & (how < 0.4)
    st["step_count"][late] = RESET_MAX_STEPS + r.integers(0, 3, size=int(late.sum()))
    return st


def reset_reference(st, case):
    """include/mgx.h, mgx_reset_done: the state after the call, and was_reset"""
    A, K, B, first_env = case.A, case.K, case.B, case.first_env
    out = {k: v.copy() for k, v in st.items()}
    done = (st["agents"][..., 4] != 0).all(1) | (st["step_count"] >= RESET_MAX_STEPS)
    for b in np.nonzero(done)[0]:
        lay = (first_env + int(b) + int(st["episode"][b]) * 7919) % K
        out["grid"][b], out["agents"][b] = st["pool_grid"][lay], st["pool_agents"][lay]
        if case.aux:
            out["aux"][b] = st["pool_aux"][lay]
    out["step_count"][done] = 0
    out["episode"][done] += 1
    return out, done.astype(np.uint8)
