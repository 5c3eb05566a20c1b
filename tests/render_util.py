"""Test infrastructure for the frame rendering (include/mgx.h mgx_render_atlas / mgx_render): the g++ build of
multigrid_amd/csrc/mgx_render.h (the host atlas), an independent NumPy composer of frames from an atlas, and the fixtures recorded
from the reference by tools/gen_render_golden.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from multigrid_amd.spec import EnvSpec

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
#: (a directory of their own: every *.npz directly under tests/golden is a rollout fixture to tests.util)
RENDER_GOLDEN = os.path.join(GOLDEN, "render")
SHIM_SRC = os.path.join(HERE, "hostshim", "render_shim.cpp")
SHIM_LIB = os.path.join(HERE, "hostshim", "libmgx_render_shim.so")
HEADER = os.path.join(os.path.dirname(HERE), "multigrid_amd", "csrc", "mgx_render.h")
TILE_SIZES = (1, 7, 8, 32)
NUM_KEYS = 2500

_lib = None
_atlases = {}


def shim():
    global _lib
    if _lib is None:
        if not os.path.exists(SHIM_LIB) or os.path.getmtime(SHIM_LIB) < max(os.path.getmtime(SHIM_SRC), os.path.getmtime(HEADER)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o",
                                   SHIM_LIB + ".tmp", SHIM_SRC])
            os.replace(SHIM_LIB + ".tmp", SHIM_LIB)
        _lib = C.CDLL(SHIM_LIB)
        _lib.shim_render_atlas.argtypes = [C.c_int, C.c_void_p]
        _lib.shim_render_trig.argtypes = [C.c_void_p, C.c_void_p]
    return _lib


def host_atlas(ts: int) -> np.ndarray:
    """u8[2500, ts, ts, 3] from the g++ build of mgx_render.h."""
    if ts not in _atlases:
        out = np.zeros((NUM_KEYS, ts, ts, 3), np.uint8)
        assert shim().shim_render_atlas(ts, out.ctypes.data) == 0
        _atlases[ts] = out
    return _atlases[ts]


# ------------------------------------------------------------------------------------------------------------- the composer
# written from the reference's behaviour, not from the header: Grid.get / WorldObj.from_array (which object a cell draws),
# Grid.render (grid.py:256-300: which agent, the tile placement) and get_full_render (base.py:707-760: the highlight mask)
_DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1))


def appearance(t, c, s):
    """(type, color, state) -> appearance index (include/mgx.h: 0 empty, 1-6 wall / goal, 7-12 floor, 13-30 door, 31-36 key,
    37-42 ball, 43-48 box, 49 lava)."""
    t, c, s = (np.asarray(v, np.int64) for v in (t, c, s))
    s = s & 3
    ok = c <= 5
    out = np.zeros(np.broadcast(t, c, s).shape, np.int64)
    out = np.where(ok & ((t == 2) | (t == 8)), 1 + c, out)
    out = np.where(ok & (t == 3), 7 + c, out)
    out = np.where(ok & (t == 4) & (s <= 2), 13 + 3 * c + s, out)
    out = np.where(ok & (t == 5), 31 + c, out)
    out = np.where(ok & (t == 6), 37 + c, out)
    out = np.where(ok & (t == 7), 43 + c, out)
    return np.where(t == 9, 49, out)


def highlight_mask(spec: EnvSpec, agents: np.ndarray, obs: np.ndarray) -> np.ndarray:
    """bool[H, W]: get_full_render's highlight_mask, transposed to [y][x]."""
    H, W, v = spec.height, spec.width, spec.view_size
    m = np.zeros((H, W), bool)
    for a in range(spec.num_agents):
        fx, fy = _DIRS[int(agents[a, 1]) & 3]
        rx, ry = -fy, fx
        tlx = int(agents[a, 2]) + fx * (v - 1) - rx * (v // 2)
        tly = int(agents[a, 3]) + fy * (v - 1) - ry * (v // 2)
        for vi, vj in np.argwhere(obs[a, :, :, 0] != 0):
            x, y = tlx - fx * vj + rx * vi, tly - fy * vj + ry * vi
            if 0 <= x < W and 0 <= y < H:
                m[y, x] = True
    return m


def keys(spec: EnvSpec, grid3: np.ndarray, agents: np.ndarray, obs) -> np.ndarray:
    """i64[H, W] atlas keys of one env: grid3 u8[H,W,3] (product layout), agents u8[A,8], obs u8[A,v,v,3] or None."""
    app = appearance(grid3[..., 0], grid3[..., 1], grid3[..., 2])
    ov = np.zeros_like(app)
    at = {}
    for a in sorted(range(spec.num_agents), key=lambda i: not agents[i, 4]):      # grid.py:281-283, last writer wins
        at[int(agents[a, 2]), int(agents[a, 3])] = a
    for (x, y), a in at.items():
        if not agents[a, 4] and agents[a, 0] <= 5:
            ov[y, x] = 1 + 4 * int(agents[a, 0]) + (int(agents[a, 1]) & 3)
    hl = highlight_mask(spec, agents, obs) if obs is not None else np.zeros(app.shape, bool)
    return (app * 25 + ov) * 2 + hl


def compose(spec: EnvSpec, grid3, agents, obs, atlas: np.ndarray) -> np.ndarray:
    """u8[H*ts, W*ts, 3]: the frame assembled from atlas tiles."""
    ts = atlas.shape[1]
    k = keys(spec, grid3, agents, obs)
    tiles = atlas[k]                                                       # [H, W, ts, ts, 3]
    return np.ascontiguousarray(tiles.transpose(0, 2, 1, 3, 4).reshape(spec.height * ts, spec.width * ts, 3))


# ------------------------------------------------------------------------------------------------------------- fixtures
def tile_fixture(ts: int):
    """(tiles u8[162, K, 2, ts, ts, 3], overlays i32[K], encodings i64[162, 3])."""
    z = np.load(os.path.join(RENDER_GOLDEN, f"render_tiles_ts{ts}.npz"))
    enc = np.array([(t, c, s) for t in range(1, 10) for c in range(6) for s in range(3)], np.int64)
    return z["tiles"], z["overlays"], enc


def frame_fixtures():
    """[(name, spec, grid u8[H,W,3], agents u8[A,8], {(ts, hl): frame})] of tests/golden/render_frames.npz."""
    z = np.load(os.path.join(RENDER_GOLDEN, "render_frames.npz"))
    out = []
    for name in z["names"]:
        name = str(name)
        spec = EnvSpec(**json.loads(str(z[f"{name}.spec"])))
        frames = {}
        for k in z.files:
            if k.startswith(name + ".ts"):
                ts, hl = k[len(name) + 3:].split("_hl")
                frames[int(ts), int(hl)] = z[k]
        out.append((name, spec, z[f"{name}.grid"], z[f"{name}.agents"], frames))
    return out
