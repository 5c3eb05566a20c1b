"""The argument checks that the launchers of the row queries share (csrc/mgx_env_rows.h: check_rows_spec, check_rows, check_rows_n),
held once for all four entry points: mgx_env_copy, mgx_state_key, mgx_action_mask, mgx_distance.  No GPU: every call returns before a
launch.  What only one call checks -- its flags, its outputs, its own bounds -- stays with that call's tests (test_env_snapshot.py,
test_state_key.py, test_action_mask.py, test_distance.py: test_c_abi_argument_validation), which take their scaffolding from here.
"""
import ctypes as C

import pytest

from multigrid_amd import EnvSpec, _lib

INV, UNS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
P = 4096                                                  # a pointer that is never dereferenced: every call returns before a launch
MEMBERS = [n for n, _ in _lib.MgxEnvRows._fields_[:-1]]
INT_MAX = 2 ** 31 - 1


def full(rows=8, **kw):
    """a state set with every member at P (16-byte aligned), but for the members named"""
    return _lib.MgxEnvRows(*[kw.get(n, P) for n in MEMBERS], rows)


def ref(x):
    return C.byref(x) if x is not None else None


def dist_query(**kw):
    return _lib.MgxDistanceC(*[kw.get(k, v) for k, v in (("type_mask", 1 << 8), ("colour_mask", 0xFF), ("agent_mask", 0), ("flags", 15),
                                                          ("points", P), ("num_points", 2))])


# One entry per launcher.  calls: f(spec, n, rows, idx, bad, bare) with `rows` in each place the call takes a state set (the other
# place, where there is one, holds a full set); bare: every pointer of the call's own is NULL too (n == 0 must not look at any).
def _copy_src(sc, n, rows, idx, bad, bare):
    other, mine = (_lib.MgxEnvRows(), None) if bare else (full(), P)
    return _lib.lib().mgx_env_copy(ref(sc), n, ref(rows), idx, ref(other), mine, mine, 0 if bare else 1, 0, bad, None)


def _copy_dst(sc, n, rows, idx, bad, bare):
    other, mine = (_lib.MgxEnvRows(), None) if bare else (full(), P)
    return _lib.lib().mgx_env_copy(ref(sc), n, ref(other), idx, ref(rows), mine, mine, 0 if bare else 1, 0, bad, None)


def _key(sc, n, rows, idx, bad, bare):
    flags, salt, keys = (0, 0, None) if bare else (3, 2 ** 64 - 1, P)
    return _lib.lib().mgx_state_key(ref(sc), n, ref(rows), idx, flags, salt, keys, bad, None)


def _mask(sc, n, rows, idx, bad, bare):
    return _lib.lib().mgx_action_mask(ref(sc), n, ref(rows), idx, 0 if bare else 1, None if bare else P + 1, bad, None)


def _dist(sc, n, rows, idx, bad, bare):
    q = dist_query(points=None, num_points=0) if bare else dist_query()
    return _lib.lib().mgx_distance(ref(sc), n, ref(rows), idx, ref(q), None if bare else P + 2, None if bare else P + 6, bad, None)


ALL_ALIGNED = (("rng", 8), ("aux", 8), ("gen_state", 8), ("agents", 4), ("cur_return", 4), ("step_count", 2), ("marker", 2),
               ("episode", 2), ("cur_length", 2), ("cells", 1))
#: name -> (calls, the spec's width, required members, (member, offset that misaligns it), item counts beyond what a launch holds).
#: mgx_distance on a side of 65: what is not refused as invalid would be refused as unsupported -- INVALID_ARGUMENT comes first.
ENTRIES = {
    "mgx_env_copy": ((_copy_src, _copy_dst), 5, ("cells", "agents", "rng", "step_count"), ALL_ALIGNED, (256 * INT_MAX + 1,)),
    "mgx_state_key": ((_key,), 5, ("cells", "agents", "rng", "step_count"),
                      (("rng", 8), ("aux", 8), ("agents", 4), ("step_count", 2), ("cells", 1)), (256 * INT_MAX + 1,)),
    "mgx_action_mask": ((_mask,), 5, ("cells", "agents"), (("aux", 8), ("agents", 4), ("cells", 1)), (256 * INT_MAX + 1,)),
    "mgx_distance": ((_dist,), 65, ("cells", "agents"), (("agents", 4), ("cells", 1)), (64 * 4 * INT_MAX + 1, 16 * 4 * INT_MAX + 1)),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_row_queries_share_their_argument_checks(entry):
    """the return codes in the header's order; no call gets as far as a launch"""
    calls, width, required, aligned, beyond = ENTRIES[entry]
    sc = EnvSpec(width, 5, 2, 3, max_steps=4).to_c()
    a = full()
    for call in calls:
        f = lambda sc_, n, rows, idx=P, bad=P, bare=False: call(sc_, n, rows, idx, bad, bare)
        assert f(None, 4, a) == INV and f(sc, -1, a) == INV and f(sc, 4, None) == INV and f(sc, 4, full(rows=-1)) == INV
        for agents in (0, 33):
            bad = EnvSpec(5, 5, 2, 3).to_c()
            bad.num_agents = agents
            assert f(bad, 0, a) == INV, agents
        bad = EnvSpec(5, 5, 2, 3).to_c()
        bad.cell_bytes = 4
        assert f(bad, 4, a) == INV
        # nothing to do: MGX_OK, whatever the members
        assert f(sc, 0, _lib.MgxEnvRows(), None, None, True) == 0 and f(sc, 0, a) == 0
        # a missing required member
        for m in required:
            assert f(sc, 4, full(**{m: None})) == INV, m
        # alignment: 16 bytes for what moves as 16-byte vectors, 8 for the 8-byte rows and the indices, 4 for i32, 2 for 16-bit cells
        for m, off in aligned:
            assert f(sc, 4, full(**{m: P + off})) == INV, m
        assert f(sc, 4, a, idx=P + 4) == INV and f(sc, 4, a, bad=P + 2) == INV
        # more items than a launch holds, more workgroups than a grid holds
        ok = EnvSpec(5, 5, 2, 3).to_c()
        for n in beyond:
            assert f(ok, n, a) == UNS, n
