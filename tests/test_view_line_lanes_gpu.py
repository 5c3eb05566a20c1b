"""GPU parity of the line map of the one-step kernels' P2 / P4 (mgx_fused.h gather_lines: one lane per view LINE, eight lanes per
view slot, passes of 8 slots): step and gen_obs against the C oracle for 1-5 agents, views of 3x3, 5x5 and 7x7, see_through_walls on
and off, agents carrying objects (tests/util.py random_state), on 16-bit and byte grids, in the throughput (64 view slots) and the
latency (32) instantiations -- at batches that leave the last wavefront 1, 7, 8, 9 and 63 view slots (a ragged last group of
padding records, a last pass that is empty, full, or one slot over) and that start a wavefront's observation bytes at every
residue mod 4.  Also run on the bounds-checked build (MGX_BOUNDS_CHECK: the line map's record reads, gathers, byte stores and reads
and staging stores inside the wavefront's LDS slice)."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (spec, batch, envs of the last wavefront or None = the batch as it is): the batch is rounded down to whole wavefronts of the
# launch geometry the library chooses, then the last wavefront's envs are added
CASES = [
    (dict(width=16, height=16, num_agents=1, view_size=7, max_steps=64), 40000, 1),                         # 1 slot
    (dict(width=16, height=16, num_agents=1, view_size=7, max_steps=64, see_through_walls=True), 40000, 7),   # 7
    (dict(width=16, height=16, num_agents=2, view_size=7, max_steps=64), 40000, 4),                         # 8
    (dict(width=16, height=16, num_agents=4, view_size=7, max_steps=64), 40000, 2),                         # 8
    (dict(width=16, height=16, num_agents=3, view_size=7, max_steps=64), 40000, 3),                         # 9
    (dict(width=6, height=6, num_agents=1, view_size=7, max_steps=30), 200000, 63),                        # 63
    (dict(width=16, height=16, num_agents=5, view_size=7, max_steps=64), 40000, 1),
    (dict(width=9, height=7, num_agents=3, view_size=5, max_steps=50), 50000, 3),                           # 9
    (dict(width=9, height=7, num_agents=2, view_size=5, max_steps=50, see_through_walls=True), 50000, 4),   # 8
    (dict(width=8, height=8, num_agents=3, view_size=3, max_steps=30), 60000, 3),                           # 9
    (dict(width=8, height=8, num_agents=1, view_size=3, max_steps=30, see_through_walls=True), 150000, 7),   # 7
    (dict(width=16, height=16, num_agents=3, view_size=7, max_steps=64, cell_bytes=3), 40000, 3),           # byte grids
    (dict(width=9, height=7, num_agents=2, view_size=5, max_steps=50, cell_bytes=3), 50000, 1),
    (dict(width=8, height=8, num_agents=4, view_size=3, max_steps=30, cell_bytes=3), 777, None),
    # small batches: the latency instantiations, wavefronts of few envs (observation bytes from every residue mod 4)
    *[(dict(width=16, height=16, num_agents=A, view_size=7, max_steps=64), 777, None) for A in (1, 2, 3, 4, 5)],
    (dict(width=9, height=7, num_agents=3, view_size=5, max_steps=50), 333, None),
    (dict(width=8, height=8, num_agents=5, view_size=3, max_steps=30), 201, None),
    # one env per wavefront (the tile fills its LDS budget) with an odd number of agents: every residue
    (dict(width=60, height=60, num_agents=3, view_size=7, max_steps=40), 301, None),
    (dict(width=64, height=48, num_agents=5, view_size=5, max_steps=40, see_through_walls=True), 203, None),
]


def geometry(kw, B, rem):
    """(spec, batch, envs per wavefront) of a case: the batch with `rem` envs in its last wavefront"""
    from multigrid_amd import EnvSpec, _lib
    spec = EnvSpec(**kw)
    if rem is not None:
        gw = _lib.launch_info(spec, B)["envs_per_wavefront"]
        B = B // gw * gw + rem
    gw = _lib.launch_info(spec, B)["envs_per_wavefront"]
    assert rem is None or rem < gw, (kw, B, gw)
    return spec, B, gw


def run_cases(check_bounds=False):
    import torch
    from multigrid_amd import BatchedMultiGridEnv, _lib
    from oracle import binding as ob
    from tests import util
    dev = "cuda:0"
    residues, last_slots = set(), set()
    for kw, B, rem in CASES:
        spec, B, gw = geometry(kw, B, rem)
        A = spec.num_agents
        last_slots.add((B % gw or gw) * A)
        residues |= {(w * gw * A * spec.view_size ** 2 * 3) % 4 for w in range((B + gw - 1) // gw)}
        name = f"{kw} B={B} Gw={gw}"
        st = util.random_state(spec, B, seed=zlib.crc32(name.encode()) % 10000)
        env = BatchedMultiGridEnv(spec, B, dev)
        env.load_state(st["grid"], st["agents"], st["rng"], st["target"], st["step_count"])
        ref = {k: v.copy() for k, v in st.items()}
        sd = spec.as_dict()
        o_ref, d_ref = ob.gen_obs_batch(sd, ref["grid"], ref["agents"], nthreads=8)
        obs, dirs = env.gen_obs()
        np.testing.assert_array_equal(obs.cpu().numpy(), o_ref, err_msg=name)
        np.testing.assert_array_equal(dirs.cpu().numpy(), d_ref, err_msg=name)
        for t in range(3):
            act = util.random_actions(B, A, seed=91 + t)
            o_ref = ob.step_batch(sd, ref["grid"], ref["agents"], ref["rng"], ref["step_count"], act, ref["target"], nthreads=8)[0]
            obs = env.step(torch.from_numpy(act).to(dev))[0]
            np.testing.assert_array_equal(obs.cpu().numpy(), o_ref, err_msg=f"{name} step {t}")
            np.testing.assert_array_equal(env.grid.cpu().numpy(), ref["grid"], err_msg=f"{name} step {t}")
            np.testing.assert_array_equal(env.agents.cpu().numpy(), ref["agents"], err_msg=f"{name} step {t}")
        env.check_errors()
        del env
    assert {1, 7, 8, 9, 63} <= last_slots, last_slots
    assert residues == {0, 1, 2, 3}, residues
    if check_bounds:
        import ctypes
        L = _lib.lib()
        v = (ctypes.c_int32 * 2)()
        assert L.mgx_debug_bounds_violations(v) == 0
        assert v[0] == 0, f"{v[0]} LDS accesses outside their wavefront's slice (last site {v[1]})"
        print(f"bounds check: {v[0]} LDS accesses outside their wavefront's slice")
    print("line lanes ok")


def test_line_lanes_vs_oracle():
    run_cases()


def test_line_lanes_on_the_bounds_checked_build():
    from multigrid_amd import build
    assert os.path.exists(build.LIB_CHK), "libmgx_chk.so is missing: __graft_entry__.build() makes it"
    code = "import sys; sys.path.insert(0, %r); from tests.test_view_line_lanes_gpu import run_cases; run_cases(True)" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, cwd=ROOT,
                         env=dict(os.environ, MGX_LIBMGX=build.LIB_CHK))
    assert out.returncode == 0 and "line lanes ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert "bounds check: 0 LDS accesses" in out.stdout, out.stdout[-500:]
