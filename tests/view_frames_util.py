"""Test infrastructure for the view frames (include/mgx.h "VIEW FRAMES": mgx_render_views, BatchedMultiGridEnv.render_views): a
NumPy composer written from the rule in the header's text (not from csrc/mgx_render.h), the g++ build of the header's key rule
(tests/hostshim/view_shim.cpp), and the frames recorded from the reference by tools/gen_view_golden.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import render_util as ru

SHIM_SRC = os.path.join(ru.HERE, "hostshim", "view_shim.cpp")
SHIM_LIB = os.path.join(ru.HERE, "hostshim", "libmgx_view_shim.so")
FIXTURE = os.path.join(ru.RENDER_GOLDEN, "view_frames.npz")
UNSEEN, AGENT = 0, 10

_lib = None


def shim():
    global _lib
    if _lib is None:
        if not os.path.exists(SHIM_LIB) or os.path.getmtime(SHIM_LIB) < max(os.path.getmtime(SHIM_SRC), os.path.getmtime(ru.HEADER)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o",
                                   SHIM_LIB + ".tmp", SHIM_SRC])
            os.replace(SHIM_LIB + ".tmp", SHIM_LIB)
        _lib = C.CDLL(SHIM_LIB)
        _lib.shim_view_keys.argtypes = [C.c_int64] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
        _lib.shim_view_keys.restype = None
    return _lib


def header_keys(cells, own, dirs, colours, highlight) -> np.ndarray:
    """i32[n]: render_view_key of the g++ build over cells u8[n,3], own / dirs / colours u8[n]."""
    cells, own, dirs, colours = (np.ascontiguousarray(a, np.uint8) for a in (cells, own, dirs, colours))
    out = np.zeros(len(cells), np.int32)
    shim().shim_view_keys(len(cells), cells.ctypes.data, own.ctypes.data, dirs.ctypes.data, colours.ctypes.data, int(highlight),
                          out.ctypes.data)
    return out


# ------------------------------------------------------------------------------------------------------------- the composer
def view_keys(obs, dirs, colours, highlight) -> np.ndarray:
    """i64[n, v, v] atlas keys, indexed [view][i][j] like the images: obs u8[n,v,v,3], dirs u8[n] (any byte: dir & 3), colours u8[n]."""
    img = np.asarray(obs, np.int64)
    n, v = img.shape[0], img.shape[1]
    t, c, s = img[..., 0], img[..., 1], img[..., 2]
    D = (np.asarray(dirs, np.int64) & 3)[:, None, None]
    col = np.asarray(colours, np.int64)
    app = ru.appearance(t, c, s)                                            # unseen, empty, agent, out of range: nothing drawn
    ov = np.where((t == AGENT) & (c <= 5), 1 + 4 * c + ((s - D + 3) & 3), 0)   # another agent, turned into the viewer's frame
    ov[:, v // 2, v - 1] = np.where(col <= 5, 1 + 4 * col + 3, 0)           # the viewer, facing up, over what it carries
    hl = (t != UNSEEN) if highlight else np.zeros(t.shape, bool)
    return (app * 25 + ov) * 2 + hl


def compose_views(obs, dirs, colours, atlas: np.ndarray, highlight: bool, channels_first: bool = False) -> np.ndarray:
    """u8[n, P, P, 3] (channels_first: u8[n, 3, P, P]): pixel (py, px) comes from the tile of image[px // ts, py // ts]."""
    ts = atlas.shape[1]
    k = view_keys(obs, dirs, colours, highlight)
    n, v = k.shape[0], k.shape[1]
    tiles = atlas[k.transpose(0, 2, 1)]                                     # [n, j, i, ts, ts, 3]: tile rows top to bottom
    out = tiles.transpose(0, 1, 3, 2, 4, 5).reshape(n, v * ts, v * ts, 3)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2) if channels_first else out)


def census(obs) -> dict:
    """What a batch of views u8[n,v,v,3] holds that the rule treats specially (a test on views with none of it shows nothing)."""
    img = np.asarray(obs)
    v = img.shape[1]
    t, c = img[..., 0].copy(), img[..., 1]
    own = t[:, v // 2, v - 1].copy()
    t[:, v // 2, v - 1] = 255
    return {"other_agents": int(((t == AGENT) & (c <= 5)).sum()), "unseen": int((t == UNSEEN).sum()),
            "carried": int(np.isin(own, (5, 6, 7)).sum())}


# ------------------------------------------------------------------------------------------------------------- fixtures
def fixture():
    """tests/golden/render/view_frames.npz: image u8[K,v,v,3], dir u8[K], colour u8[K], frames {(ts, highlight): u8[K,P,P,3]}."""
    z = np.load(FIXTURE)
    frames = {(8, 1): z["frames_ts8_hl1"], (7, 0): z["frames_ts7_hl0"]}
    return z["image"], z["dir"], z["colour"], frames
