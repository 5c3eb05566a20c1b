"""The streaming kernels of csrc/mgx_aux.hip -- one_hot, full_obs, pack_grid*, unpack_grid*, check_grid, reset_done -- through every
alignment, group and tail path, against plain NumPy references written from the words of include/mgx.h (tests/aux_cases.py).

Every assertion is byte-exact.  The C ABI is called directly (ctypes) so that pointers can be offset; every tensor the kernels touch
sits between guard bytes that must come back unchanged.  Which kernel paths the cases reach is derived and asserted on the CPU by
tests/test_aux_branch_census.py.

The other kernels of that file -- the persistent hand-shake's producers persistent_post, persistent_wait and persistent_feed -- are
walked the same way by tests/test_persist_producers_gpu.py, which borrows `Buf` from here (cases: tests/persist_cases.py, census:
tests/test_persist_branch_census.py, refusals: tests/test_persist_refusals.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from multigrid_amd import EnvSpec, _lib, layouts
from tests import aux_cases as ac

DEV = "cuda:0"
gpu = pytest.mark.gpu
GUARD, FILL = 256, 0xA5
INT_MAX = 2 ** 31 - 1


class Buf:
    """n bytes on the device at `off` bytes past a 256-byte boundary, between two guards"""

    def __init__(self, n, off=0, data=None):
        self.n, self.off = int(n), off
        self.t = torch.full((GUARD + off + self.n + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + GUARD + off
        if data is not None:
            raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
            assert raw.size == self.n
            self.t[GUARD + off:GUARD + off + self.n] = torch.from_numpy(raw).to(DEV)

    def get(self, dtype=np.uint8):
        return self.t[GUARD + self.off:GUARD + self.off + self.n].cpu().numpy().view(dtype)

    def guards_intact(self):
        lo, hi = self.t[:GUARD + self.off].cpu().numpy(), self.t[GUARD + self.off + self.n:].cpu().numpy()
        return bool((lo == FILL).all() and (hi == FILL).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


def c_spec(W, H, A, cb, max_steps=ac.RESET_MAX_STEPS):
    return EnvSpec(W, H, A, 3, max_steps=max_steps, cell_bytes=cb).to_c()


# ===================================================================================================================== full_obs
@gpu
@pytest.mark.parametrize("case", ac.FULL_OBS, ids=ac.FULL_OBS_IDS)
def test_full_obs_whole_output_and_guard(case):
    L = _lib.lib()
    cells, g3, ag = ac.full_obs_inputs(case)
    want = ac.full_obs_reference(g3, ag)
    d_cells, d_ag, d_out = Buf(cells.nbytes, data=cells), Buf(ag.nbytes, data=ag), Buf(want.nbytes)
    sc = c_spec(case.W, case.H, case.A, case.cb)
    assert L.mgx_full_obs(C.byref(sc), case.B, d_cells.ptr, d_ag.ptr, d_out.ptr, stream()) == 0
    got = d_out.get().reshape(want.shape)
    if not np.array_equal(got, want):
        envs = np.nonzero((got != want).reshape(case.B, -1).any(1))[0]
        b = int(envs[0])
        pytest.fail(f"{len(envs)} envs differ; the first is env {b} = env {b % case.G} of wavefront {b // case.G} (G = {case.G}):\n"
                    f"got {got[b].reshape(-1, 3).tolist()}\nwant {want[b].reshape(-1, 3).tolist()}\nagents {ag[b].tolist()}")
    assert d_out.guards_intact() and d_cells.guards_intact() and d_ag.guards_intact()


# ===================================================================================================================== one_hot
def one_hot_cells(r, n):
    """bytes from 0..255, three quarters of them small enough to land inside a field now and then"""
    small = r.integers(0, 32, size=(n, 3), dtype=np.uint8)
    return np.where(r.random(size=(n, 3)) < 0.75, small, r.integers(0, 256, size=(n, 3), dtype=np.uint8))


def run_one_hot(L, cells, dims, off):
    n, D = cells.shape[0], sum(dims)
    d_in, d_out = Buf(n * 3, off, cells), Buf(n * D)
    ds = (C.c_int32 * 3)(*dims)
    assert L.mgx_one_hot(d_in.ptr, n, ds, d_out.ptr, stream()) == 0
    got = d_out.get().reshape(n, D)
    want = ac.one_hot_reference(cells, dims)
    if not np.array_equal(got, want):
        c = int(np.nonzero((got != want).any(1))[0][0])
        pytest.fail(f"one_hot dims {dims} n {n} input offset {off}: cell {c} = {cells[c].tolist()}: got {got[c].tolist()} want {want[c].tolist()}")
    assert d_out.guards_intact(), f"one_hot dims {dims} n {n} input offset {off}: wrote outside out"


@gpu
def test_one_hot_every_dims_up_to_32_channels():
    """every (d0, d1, d2) with D in {3, 4, 15, 16, 17, 21, 31, 32}: two chunks with a ragged second one, the input offset going round"""
    L = _lib.lib()
    r = ac._rng("one_hot dims")
    for k, dims in enumerate(ac.one_hot_dims()):
        n = 1025 + k % 7
        run_one_hot(L, one_hot_cells(r, n), dims, k % 4)


@gpu
@pytest.mark.parametrize("dims", ac.ONE_HOT_SWEEP_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_one_hot_sizes_around_the_chunk_and_input_offsets(dims):
    L = _lib.lib()
    r = ac._rng("one_hot n", dims)
    for n in ac.ONE_HOT_N:
        cells = one_hot_cells(r, n)
        for off in range(4):
            run_one_hot(L, cells, dims, off)


@gpu
@pytest.mark.parametrize("off", [0, 3])
def test_one_hot_grid_stride_loop_at_a_ragged_size(off):
    n, dims = ac.ONE_HOT_BIG
    run_one_hot(_lib.lib(), ac._rng("one_hot big").integers(0, 4, size=(n, 3), dtype=np.uint8), dims, off)


def test_one_hot_refuses_33_channels_and_a_misaligned_out():
    """(argument checks run before any HIP call: no device needed)"""
    L = _lib.lib()
    for dims in ((11, 11, 11), (31, 1, 1), (1, 1, 31)):
        assert L.mgx_one_hot(4096, 8, (C.c_int32 * 3)(*dims), 4096, None) == _lib.ERR_UNSUPPORTED
    for off in (1, 2, 4, 8, 15):
        assert L.mgx_one_hot(4096, 8, (C.c_int32 * 3)(11, 6, 4), 4096 + off, None) == _lib.ERR_INVALID_ARGUMENT
    assert L.mgx_one_hot(4096, 8, (C.c_int32 * 3)(11, 0, 4), 4096, None) == _lib.ERR_INVALID_ARGUMENT


# ===================================================================================================================== pack / unpack
def check_packed(got, g, valid, pack, ctx):
    """the packed values on the cells the format can hold (the others are stored truncated: unspecified)"""
    want = pack(g[valid])
    if not np.array_equal(got[valid], want):
        k = int(np.nonzero(got[valid] != want)[0][0])
        pytest.fail(f"{ctx}: valid cell {g[valid][k].tolist()} packed as {int(got[valid][k]):#x}, want {int(want[k]):#x}")


@gpu
def test_pack_grid_and_unpack_grid_tails_and_offsets():
    L = _lib.lib()
    r = ac._rng("pack flat")
    for n in ac.PACK_N:
        g = ac.pack_cells3(r, (n,))
        valid = ac.valid16(g)
        for s_off in range(8):
            for d_off in (0, 2, 8):
                ctx = f"pack_grid n {n} source +{s_off} destination +{d_off}"
                d_in, d_out, d_bad = Buf(n * 3, s_off, g), Buf(n * 2, d_off), Buf(8, data=np.zeros(2, np.int32))
                assert L.mgx_pack_grid(d_in.ptr, n, d_out.ptr, d_bad.ptr, stream()) == 0
                assert d_bad.get(np.int32).tolist() == [int((~valid).sum()), 0], ctx
                got = d_out.get(np.uint16)
                check_packed(got, g, valid, layouts.pack_cells, ctx)
                assert d_out.guards_intact() and d_bad.guards_intact(), ctx
                # back again: the source misaligned as the packed cells are, the destination as the bytes were
                d_back = Buf(n * 3, s_off)
                assert L.mgx_unpack_grid(d_out.ptr, n, d_back.ptr, stream()) == 0
                np.testing.assert_array_equal(d_back.get().reshape(n, 3)[valid], g[valid], err_msg=ctx)
                assert d_back.guards_intact(), ctx
        d_in, d_out = Buf(n * 3, 0, g), Buf(n * 2)
        assert L.mgx_pack_grid(d_in.ptr, n, d_out.ptr, None, stream()) == 0                            # (bad may be NULL)
        check_packed(d_out.get(np.uint16), g, valid, layouts.pack_cells, f"pack_grid n {n} without bad")


@gpu
@pytest.mark.parametrize("wide", [True, False], ids=["unpack_grid", "unpack_grid8"])
def test_unpack_every_bit_pattern_tails_and_offsets(wide):
    """unpack is defined on every 16-bit / 8-bit value (layouts.unpack_cells / unpack_cells8 say the same in NumPy)"""
    L = _lib.lib()
    r = ac._rng("unpack", wide)
    for n in ac.PACK_N:
        p = r.integers(0, 1 << 16, size=n).astype(np.uint16) if wide else r.integers(0, 256, size=n, dtype=np.uint8)
        want = layouts.unpack_cells(p) if wide else layouts.unpack_cells8(p)
        for s_off in ((0, 2, 8, 14) if wide else (0, 1, 4, 7)):
            for d_off in range(8):
                d_in, d_out = Buf(p.nbytes, s_off, p), Buf(n * 3, d_off)
                rc = (L.mgx_unpack_grid if wide else L.mgx_unpack_grid8)(d_in.ptr, n, d_out.ptr, stream())
                assert rc == 0
                np.testing.assert_array_equal(d_out.get().reshape(n, 3), want, err_msg=f"n {n} source +{s_off} destination +{d_off}")
                assert d_out.guards_intact()


@gpu
@pytest.mark.parametrize("compact", [False, True], ids=["pack_grid_env", "pack_grid8_env"])
@pytest.mark.parametrize("W,H,B", ac.PACK_ENV, ids=[f"{w}x{h}_B{b}" for w, h, b in ac.PACK_ENV])
def test_pack_env_counts_values_and_round_trip(W, H, B, compact):
    L = _lib.lib()
    r = ac._rng("pack env", W, H, B, compact)
    g = ac.pack_env_cells3(r, B, H, W, compact)
    n = B * H * W
    valid = (ac.valid8 if compact else ac.valid16)(g)
    want_bad = [int((~valid).sum()), ac.ring_bad(g)]
    assert B == 1 or (want_bad[0] > 0 and want_bad[1] > 0 and valid.sum() > n // 4)
    pack, cellb = (layouts.pack_cells8, 1) if compact else (layouts.pack_cells, 2)
    fn, unfn = (L.mgx_pack_grid8_env, L.mgx_unpack_grid8) if compact else (L.mgx_pack_grid_env, L.mgx_unpack_grid)
    for s_off in range(8):
        for d_off in ((0, 1, 4) if compact else (0, 2, 8)):
            ctx = f"{W}x{H} B {B} source +{s_off} destination +{d_off}"
            d_in, d_out, d_bad = Buf(n * 3, s_off, g), Buf(n * cellb, d_off), Buf(8, data=np.zeros(2, np.int32))
            assert fn(d_in.ptr, B, H, W, d_out.ptr, d_bad.ptr, stream()) == 0
            assert d_bad.get(np.int32).tolist() == want_bad, ctx
            got = d_out.get(np.uint8 if compact else np.uint16).reshape(B, H, W)
            check_packed(got, g, valid, pack, ctx)
            assert d_out.guards_intact() and d_bad.guards_intact() and d_in.guards_intact(), ctx
            d_back = Buf(n * 3, (s_off + 3) % 8)
            assert unfn(d_out.ptr, n, d_back.ptr, stream()) == 0
            np.testing.assert_array_equal(d_back.get().reshape(B, H, W, 3)[valid], g[valid], err_msg=ctx)
            assert d_back.guards_intact(), ctx


# ===================================================================================================================== check_grid
def run_check(L, case, cells, ag):
    d_cells, d_bad = Buf(cells.nbytes, data=cells), Buf(16, data=np.array([0, 0, 0, INT_MAX], np.int32))
    d_ag = Buf(ag.nbytes, data=ag) if ag is not None else None
    sc = c_spec(case.W, case.H, case.A, case.cb)
    assert L.mgx_check_grid(C.byref(sc), case.B, d_cells.ptr, d_ag.ptr if ag is not None else None, d_bad.ptr, stream()) == 0
    assert d_bad.guards_intact()
    return d_bad.get(np.int32).tolist()


@gpu
@pytest.mark.parametrize("case", ac.CHECK, ids=ac.CHECK_IDS)
def test_check_grid_counts_dense_defects_of_every_class(case):
    L = _lib.lib()
    W, H, A, B, cb = case
    cells, ag = ac.check_inputs(case)
    want = ac.check_reference(cells, ag, W, H, cb)
    assert min(want[:3]) > 0
    assert run_check(L, case, cells, ag) == want
    assert run_check(L, case, cells, None) == ac.check_reference(cells, None, W, H, cb)              # agents = NULL: not looked at
    # a clean state; then one violation, in the last env only: a cell, a ring cell, an agent row
    clean, rows = ac.valid_state(ac._rng("clean", *case), W, H, A, B, cb)
    assert run_check(L, case, clean, rows) == [0, 0, 0, INT_MAX]
    bits = 8 * cb
    one = clean.copy()
    one[B - 1, H - 2, W - 2] ^= 1 << (bits - 1)                                                     # its opaque bit
    assert run_check(L, case, one, rows) == [1, 0, 0, B - 1] == ac.check_reference(one, rows, W, H, cb)
    one = clean.copy()
    one[B - 1, H - 1, W - 1] = clean[0, 1, 1] if clean[0, 1, 1] != clean[0, 0, 0] else 1
    want = ac.check_reference(one, rows, W, H, cb)
    assert want[1] == 1 and want[3] == B - 1 and run_check(L, case, one, rows) == want
    late = rows.copy()
    late[B - 1, A - 1, 2] = 0                                                                       # stands on the ring
    assert run_check(L, case, clean, late) == [0, 0, 1, B - 1]
    late[0, 0, 1] = 4                                                                               # ... and env 0: a direction
    assert run_check(L, case, clean, late) == [0, 0, 2, 0]


# ===================================================================================================================== reset_done
@gpu
@pytest.mark.parametrize("case", ac.RESET, ids=ac.RESET_IDS)
def test_reset_done_partial_subsets_through_every_copy_unit(case):
    L = _lib.lib()
    st = ac.reset_inputs(case)
    want, was = ac.reset_reference(st, case)
    d = {k: Buf(v.nbytes, case.pool_off if k == "pool_grid" else 0, v) for k, v in st.items()}
    d_was = Buf(case.B) if case.A != 4 else None                                                    # (was_reset may be NULL)
    sc = c_spec(case.W, case.H, case.A, case.cb)
    rc = L.mgx_reset_done(C.byref(sc), case.B, case.first_env, case.K, d["pool_grid"].ptr, d["pool_agents"].ptr,
                          d["pool_aux"].ptr if case.aux else None, d["grid"].ptr, d["agents"].ptr, d["step_count"].ptr,
                          d["aux"].ptr if case.aux else None, d["episode"].ptr, d_was.ptr if d_was else None, stream())
    assert rc == 0
    for k, v in want.items():                                                                       # (untouched envs included)
        got = d[k].get(v.dtype).reshape(v.shape)
        if not np.array_equal(got, v):
            b = int(np.nonzero((got != v).reshape(v.shape[0], -1).any(1))[0][0])
            pytest.fail(f"{k}: entry {b} differs (finished: {bool(was[b]) if k not in ('pool_grid', 'pool_agents', 'pool_aux') else '-'})")
        assert d[k].guards_intact(), k
    if d_was:
        np.testing.assert_array_equal(d_was.get(), was)
        assert d_was.guards_intact()
