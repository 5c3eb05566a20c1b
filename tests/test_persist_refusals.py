"""What mgx_persistent_post, mgx_persistent_wait and mgx_persistent_feed refuse (include/mgx.h), through the C ABI.  The argument checks
run before any HIP call, so no device is needed: the pointers below are plain numbers that nothing dereferences."""
import ctypes as C

import pytest

from multigrid_amd import EnvSpec, _lib
from tests import hostshim

INVALID, UNSUPPORTED = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
ACT, GR, DONE, CTRL, TRACE = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000       # (each aligned to 64 KiB)


def c_spec(A):
    sc = EnvSpec(16, 16, min(max(A, 1), 32), 3).to_c()
    sc.num_agents = A                           # (0 and 33: what EnvSpec itself would not build)
    return sc


def post(A=4, batch=8, actions=ACT, step=1, granules=GR):
    return _lib.lib().mgx_persistent_post(C.byref(c_spec(A)), batch, actions, step, granules, None)


def wait(done=DONE, waves=8, step=1, ctrl=CTRL, timeout_ms=100):
    return _lib.lib().mgx_persistent_wait(done, waves, step, ctrl, timeout_ms, None)


def feed(A=4, batch=8, actions=ACT, steps=2, granules=GR, done=DONE, ctrl=CTRL, timeout_ms=100, waves=8, trace=TRACE, p=True):
    pers = _lib.MgxPersistent(granules, done, ctrl, steps, timeout_ms)
    return _lib.lib().mgx_persistent_feed(C.byref(c_spec(A)), batch, actions, steps, C.byref(pers) if p else None, waves, trace, None)


def test_post_refuses():
    assert post(actions=None) == INVALID and post(granules=None) == INVALID
    assert post(step=0) == INVALID
    assert post(granules=GR + 4) == INVALID
    for A in (4, 8):
        for off in (1, 2):
            assert post(A=A, actions=ACT + off) == INVALID, (A, off)
    assert post(batch=0) == INVALID
    assert post(A=0) == INVALID and post(A=33) == INVALID
    assert _lib.lib().mgx_persistent_post(None, 8, ACT, 1, GR, None) == INVALID


def test_wait_refuses():
    assert wait(done=None) == INVALID and wait(ctrl=None) == INVALID
    assert wait(waves=0) == INVALID
    assert wait(timeout_ms=0) == INVALID and wait(timeout_ms=30001) == INVALID


def test_feed_refuses():
    assert feed(actions=None) == INVALID and feed(granules=None) == INVALID
    assert feed(granules=GR + 4) == INVALID
    for A in (4, 8):
        for off in (1, 2):
            assert feed(A=A, actions=ACT + off) == INVALID, (A, off)
    assert feed(batch=0) == INVALID
    assert feed(A=0) == INVALID and feed(A=33) == INVALID
    assert feed(done=None) == INVALID and feed(ctrl=None) == INVALID
    assert feed(steps=0) == INVALID
    assert feed(waves=0) == INVALID
    assert feed(timeout_ms=0) == INVALID and feed(timeout_ms=30001) == INVALID
    assert feed(trace=TRACE + 4) == INVALID
    assert feed(p=False) == INVALID


def test_feed_refuses_an_odd_action_pointer_at_two_agents():
    """persistent_feed_kernel<2> reads the action tensor as 16-bit words"""
    assert feed(A=2, actions=ACT + 1) == INVALID and feed(A=2, actions=ACT + 3) == INVALID


@pytest.mark.parametrize("A,limit", [(4, 2 ** 31), (17, 2 ** 30), (25, 1_431_655_766)], ids=["gpe1", "gpe5", "gpe7"])
def test_granule_limits_through_the_abi(A, limit):
    """MGX_ERR_UNSUPPORTED from `limit` granules on (include/mgx.h; tests/test_recip32.py derives the limits); one granule below,
    the limit is not what refuses the call -- a NULL pointer is"""
    gpe = (A + 3) // 4
    over = -(-limit // gpe)                     # the first batch with >= limit granules
    assert hostshim.granule_geometry(A, over)[0] == UNSUPPORTED and hostshim.granule_geometry(A, over - 1)[0] == 0
    assert post(A=A, batch=over) == UNSUPPORTED and feed(A=A, batch=over) == UNSUPPORTED
    assert post(A=A, batch=over - 1, actions=None) == INVALID and feed(A=A, batch=over - 1, actions=None) == INVALID
