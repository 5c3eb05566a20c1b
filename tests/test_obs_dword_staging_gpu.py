"""GPU parity of the one-step kernels' dword staging of the observation (mgx_fused_body.inc P4/P5, views of one lane pass): the
step and gen_obs against the oracle for 1-5 agents (and 9 / 13, one env per wavefront) at batches that are not multiples of the
envs per wavefront, on 16-bit and compact cells, in the throughput and the latency instantiations -- so that a wavefront's
observation bytes start at every residue mod 4 (o0 = first (env, agent) row x V*V*3) and last waves are partial.  Also run on
the bounds-checked build (MGX_BOUNDS_CHECK: every staging store and read inside the wavefront's LDS slice)."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (spec, batch): small batches take the latency instantiations, large ones the throughput ones
CASES = [
    *[(dict(width=16, height=16, num_agents=A, view_size=7, max_steps=64), B) for A in (1, 2, 3, 4, 5) for B in (777, 40003)],
    (dict(width=9, height=7, num_agents=3, view_size=5, max_steps=50), 50001),
    (dict(width=8, height=8, num_agents=5, view_size=3, max_steps=30, see_through_walls=True), 30001),
    (dict(width=12, height=12, num_agents=9, view_size=5, max_steps=40), 333),
    (dict(width=12, height=12, num_agents=13, view_size=7, max_steps=40), 201),
    (dict(width=16, height=16, num_agents=3, view_size=7, max_steps=64, cell_bytes=1), 40003),
    (dict(width=16, height=16, num_agents=5, view_size=5, max_steps=64, cell_bytes=1), 999),
]


def run_cases(check_bounds=False):
    import torch
    from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib
    from oracle import binding as ob
    from tests import util
    dev = "cuda:0"
    residues = set()
    for kw, B in CASES:
        spec = EnvSpec(**kw)
        info = _lib.launch_info(spec, B)
        gw, A = info["envs_per_wavefront"], spec.num_agents
        residues |= {(w * gw * A * spec.view_size ** 2 * 3) % 4 for w in range((B + gw - 1) // gw)}
        name = f"{kw} B={B} Gw={gw}"
        st = util.random_state(spec, B, seed=zlib.crc32(name.encode()) % 10000)
        env = BatchedMultiGridEnv(spec, B, dev)
        env.load_state(st["grid"], st["agents"], st["rng"], st["target"], st["step_count"])
        ref = {k: v.copy() for k, v in st.items()}
        sd = spec.as_dict()
        o_ref, _ = ob.gen_obs_batch(sd, ref["grid"], ref["agents"], nthreads=8)
        obs, _ = env.gen_obs()
        np.testing.assert_array_equal(obs.cpu().numpy(), o_ref, err_msg=name)
        for t in range(3):
            act = util.random_actions(B, A, seed=77 + t)
            o_ref = ob.step_batch(sd, ref["grid"], ref["agents"], ref["rng"], ref["step_count"], act, ref["target"], nthreads=8)[0]
            obs = env.step(torch.from_numpy(act).to(dev))[0]
            np.testing.assert_array_equal(obs.cpu().numpy(), o_ref, err_msg=f"{name} step {t}")
            np.testing.assert_array_equal(env.agents.cpu().numpy(), ref["agents"], err_msg=f"{name} step {t}")
        env.check_errors()
        del env
    assert residues == {0, 1, 2, 3}, residues
    if check_bounds:
        import ctypes
        L = _lib.lib()
        v = (ctypes.c_int32 * 2)()
        assert L.mgx_debug_bounds_violations(v) == 0
        assert v[0] == 0, f"{v[0]} LDS accesses outside their wavefront's slice (last site {v[1]})"
        print(f"bounds check: {v[0]} LDS accesses outside their wavefront's slice")
    print("dword staging ok")


def test_dword_staging_vs_oracle():
    run_cases()


def test_dword_staging_on_the_bounds_checked_build():
    from multigrid_amd import build
    assert os.path.exists(build.LIB_CHK), "libmgx_chk.so is missing: __graft_entry__.build() makes it"
    code = "import sys; sys.path.insert(0, %r); from tests.test_obs_dword_staging_gpu import run_cases; run_cases(True)" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, cwd=ROOT,
                         env=dict(os.environ, MGX_LIBMGX=build.LIB_CHK))
    assert out.returncode == 0 and "dword staging ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert "bounds check: 0 LDS accesses" in out.stdout, out.stdout[-500:]
