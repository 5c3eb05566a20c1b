"""ctypes access to tests/hostshim/hostshim.cpp (test infrastructure; see the .cpp header)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libmgx_hostshim.so")
SRC = os.path.join(HERE, "hostshim.cpp")
RULES = os.path.join(os.path.dirname(os.path.dirname(HERE)), "multigrid_amd", "csrc", "mgx_rules.h")
GEOM = os.path.join(os.path.dirname(RULES), "mgx_aux_geom.h")

_lib = None


def lib():
    global _lib
    if _lib is None:
        if os.environ.get("MGX_SANITIZE") == "1":           # tests/test_checked_build.py: ASan + UBSan build, kept elsewhere
            out = os.path.join(os.environ.get("MGX_SANITIZE_DIR", "/tmp"), "libmgx_hostshim_san.so")
            subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall",
                                   "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out, SRC])
            _lib = C.CDLL(out)
            return _lib
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(RULES), os.path.getmtime(GEOM)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall",
                                   "-o", LIB, SRC])
        _lib = C.CDLL(LIB)
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _layouts():
    from multigrid_amd import layouts
    return layouts


FORMS = {"prefix": 0, "first": 1}
PATH_PAIRS = 64


def step_env(spec, tile, rows8, act, rng4, step_count, target, force_serial=False, hook_order=None, form="prefix", path=False):
    """tile u8[H,W,3], rows8 u8[A,8], act i8[A], rng4 u64[4], target = aux u8[16]; all updated in place.
    Returns dict(obs, reward, terminated, truncated, order, rc, n_dirty).

    form: which of the kernel's two fallback commits is modelled (mgx_fused_body.inc, P1s): "prefix" -- the agents ranked below the
    first blocked one commit with their order-free results (the kernels with PREFIX, at A > 2); "first" -- only the agent visited
    first commits early, and only without an unknown action or an event (every other kernel, and every kernel at A <= 2).
    path=True adds `path` to the result: what the decision logic did for this env --
        fallback (bool), why (set of "bad", "conflict", "presence", "forced"), ends_all / ends_self (an event of that kind in the
        order-free evaluation), event_cutoff (rank, None without one) and suppressed (agents with an effective action -- one that
        would have moved, turned or written -- behind it) in the no-fallback branch, commit_cutoff (the rank the sequential loop
        starts at; None without fallback), pairs: [(writer's action, reader's action, front cell type, its state, box holds something)]."""
    sc = spec.to_c()
    A, v = spec.num_agents, spec.view_size
    # the rules work on packed cells (include/mgx.h MgxCell, or MgxCell8 for spec.cell_bytes == 1); the tests speak (type, color,
    # state) bytes
    L = _layouts()
    tile3, tile = tile, np.ascontiguousarray(L.pack_cells_for(spec, tile))
    over = np.empty_like(tile)
    rew = np.empty(A, np.float64); term = np.empty(A, np.uint8); trunc = np.zeros(1, np.uint8)
    order = np.empty(A, np.uint8); nd = C.c_int32(0); scnt = C.c_int32(int(step_count))
    rows = rows8.view(np.uint64).reshape(A)
    pw = np.zeros(8 + 4 * PATH_PAIRS, np.int32) if path else None
    rc = lib().shim_step_env(C.byref(sc), _p(tile, C.c_uint8), _p(over, C.c_uint8), _p(rows, C.c_uint64),
                             _p(act, C.c_int8), _p(rng4, C.c_uint64), C.byref(scnt), _p(target, C.c_uint8),
                             _p(rew, C.c_double), _p(term, C.c_uint8), _p(trunc, C.c_uint8), _p(order, C.c_uint8),
                             C.byref(nd), int(force_serial),
                             _p(np.ascontiguousarray(hook_order, dtype=np.uint8), C.c_uint8) if hook_order is not None else None,
                             FORMS[form], _p(pw, C.c_int32) if path else None)
    obs = np.empty((A, v, v, 3), np.uint8)
    assert lib().shim_obs_env(C.byref(sc), _p(over, C.c_uint8), _p(rows, C.c_uint64), _p(obs, C.c_uint8)) == 0
    assert np.array_equal(L.pack_cells_for(spec, L.unpack_cells_for(spec, tile)), tile), "opaque bits out of date"
    tile3[...] = L.unpack_cells_for(spec, tile)
    out = dict(obs=obs, reward=rew, terminated=term, truncated=int(trunc[0]), order=order, rc=rc,
               n_dirty=nd.value, step_count=scnt.value, serial=nd.value < 0)
    if path:
        assert pw[6] <= PATH_PAIRS
        why = {n for bit, n in ((1, "bad"), (2, "conflict"), (4, "presence"), (8, "forced")) if pw[1] & bit}
        out["path"] = dict(fallback=bool(pw[0]), why=why, ends_all=bool(pw[2] & 1), ends_self=bool(pw[2] & 2),
                           event_cutoff=None if pw[3] < 0 else int(pw[3]), suppressed=int(pw[4]),
                           commit_cutoff=None if pw[5] < 0 else int(pw[5]), form=form,
                           pairs=[(int(pw[8 + 4 * k]), int(pw[9 + 4 * k]), int(pw[10 + 4 * k]), int(pw[11 + 4 * k]) & 0xff, bool(pw[11 + 4 * k] >> 8))
                                  for k in range(pw[6])])
    return out


def obs_env(spec, tile, rows8):
    sc = spec.to_c()
    A, v = spec.num_agents, spec.view_size
    over = np.ascontiguousarray(_layouts().pack_cells_for(spec, tile))
    rows = np.ascontiguousarray(rows8).view(np.uint64).reshape(A)
    lib().shim_overlay(C.byref(sc), _p(over, C.c_uint8), _p(rows, C.c_uint64))
    obs = np.empty((A, v, v, 3), np.uint8)
    assert lib().shim_obs_env(C.byref(sc), _p(over, C.c_uint8), _p(rows, C.c_uint64), _p(obs, C.c_uint8)) == 0
    return obs


def full_obs_geom(W, H, cb, batch):
    """mgx_full_obs' launch geometry (csrc/mgx_aux_geom.h), or None where the launcher answers UNSUPPORTED."""
    out = np.zeros(7, np.int64)
    if not lib().shim_full_obs_geom(int(W), int(H), int(cb), C.c_int64(int(batch)), _p(out, C.c_int64)):
        return None
    return dict(zip(("G", "in_buf", "out_buf", "wave_lds", "wpb", "nwaves", "blocks"), (int(v) for v in out)))


def reset_unit(env_bytes, grid_addr=0, pool_addr=0):
    """mgx_reset_done's copy unit for a layout of `env_bytes` at these base addresses: (unit bytes, units per env)."""
    out = np.zeros(2, np.int32)
    lib().shim_reset_unit(int(env_bytes), C.c_uint64(int(grid_addr)), C.c_uint64(int(pool_addr)), _p(out, C.c_int32))
    return int(out[0]), int(out[1])


def one_hot_geom(n_cells):
    """mgx_one_hot's launch: (cells per chunk, chunks, workgroups)."""
    out = np.zeros(3, np.int64)
    lib().shim_one_hot_geom(C.c_int64(int(n_cells)), _p(out, C.c_int64))
    return tuple(int(v) for v in out)


def recip32(d):
    """ceil(2^32 / d) as the launchers compute it (csrc/mgx_aux_geom.h), d >= 2"""
    f = lib().shim_recip32
    f.restype = C.c_uint32
    return int(f(C.c_uint32(int(d))))


def recip32_exact_below(d):
    """the first n the header does NOT promise __umulhi(n, recip32(d)) == n // d for"""
    f = lib().shim_recip32_exact_below
    f.restype = C.c_uint64
    return int(f(C.c_uint32(int(d))))


def granule_geometry(num_agents, batch):
    """mgx_persistent_post / _feed's granule arithmetic: (return code, granules per env, their reciprocal, granules in all)"""
    out = np.zeros(3, np.int64)
    rc = lib().shim_granule_geometry(int(num_agents), C.c_int64(int(batch)), _p(out, C.c_int64))
    return (int(rc),) + tuple(int(v) for v in out)


def feed_geometry(ng_all):
    """mgx_persistent_feed's launch for `ng_all` granules (csrc/mgx_aux_geom.h): dict(nwg, per_wg, slice, threads, pre, max_wgs)"""
    out = np.zeros(6, np.int64)
    lib().shim_feed_geometry(C.c_int64(int(ng_all)), _p(out, C.c_int64))
    return dict(zip(("nwg", "per_wg", "slice", "threads", "pre", "max_wgs"), (int(v) for v in out)))


def feed_first_empty_slice(lo, hi):
    """the first ng_all in [lo, hi] whose launch holds a workgroup without granules, or None"""
    f = lib().shim_feed_first_empty_slice
    f.restype = C.c_int64
    v = int(f(C.c_int64(int(lo)), C.c_int64(int(hi))))
    return None if v < 0 else v


def wait_geometry():
    """persistent_wait's pass (csrc/mgx_aux_geom.h): (loads per thread, threads, flags per pass)"""
    out = np.zeros(3, np.int32)
    lib().shim_wait_geometry(_p(out, C.c_int32))
    return tuple(int(v) for v in out)
