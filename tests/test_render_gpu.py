"""Frame rendering on the MI355X (include/mgx.h mgx_render_atlas / mgx_render, BatchedMultiGridEnv.render): the device atlas
against the g++ build of the same header, frames against the reference's recorded frames in every cell format and both store
paths, frames of stepped random states and of the 255x255 grid against the NumPy composer, and no side effects."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, layouts, ops
from oracle import binding as ob
from tests import render_util as ru
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMATS = (2, 1, 3)


def _for_format(grid, agents, cb):
    """Compact cells hold no box contents (include/mgx.h MgxCell8): those are dropped -- a box draws the same whatever it holds."""
    grid, agents = grid.copy(), agents.copy()
    if cb == 1:
        grid[..., 2] = np.where(grid[..., 0] == 7, grid[..., 2] & 3, grid[..., 2])
        agents[..., 7] = np.where(agents[..., 5] == 7, agents[..., 7] & 3, agents[..., 7])
    return grid, agents


def _composed(spec, grid, agents, ts, highlight):
    obs = ob.gen_obs_batch(spec.as_dict(), grid, agents)[0] if highlight else [None] * len(grid)
    return np.stack([ru.compose(spec, grid[b], agents[b], obs[b], ru.host_atlas(ts)) for b in range(len(grid))])


@pytest.mark.parametrize("ts", (1, 7, 8, 32, 64))
def test_device_atlas_equals_host_atlas(ts):
    atlas = ops.HipBackend(EnvSpec(8, 8, 1, 7, max_steps=10), DEV).render_atlas(ts).cpu().numpy()
    want = ru.host_atlas(ts)
    bad = np.nonzero((atlas != want).any(axis=(1, 2, 3)))[0]
    assert not len(bad), f"{len(bad)} atlas tiles differ at ts={ts}: keys {bad[:10]}"


@pytest.mark.parametrize("stores", ("nt", "plain"))
@pytest.mark.parametrize("cb", FORMATS, ids=lambda c: f"cb{c}")
def test_frames_equal_recorded_frames(cb, stores, monkeypatch):
    """Each fixture state sits at a random place of a batch of random states of its spec; an env_ids permutation picks the
    envs, the fixture's frame must equal the reference's bytes and the others the composer's."""
    monkeypatch.setenv("MGX_RENDER_STORES", stores)
    for k, (name, spec0, grid, agents, frames) in enumerate(ru.frame_fixtures()):
        spec = dataclasses.replace(spec0, cell_bytes=cb)
        B = 6
        st = util.random_state(spec0, B, seed=100 + k, terminated_p=0.2)
        at = k % B
        st["grid"][at], st["agents"][at] = grid, agents
        g, a = _for_format(st["grid"], st["agents"], cb)
        env = BatchedMultiGridEnv(spec, B, DEV)
        env.load_state(g, a, validate=False)
        perm = torch.from_numpy(np.random.default_rng(k).permutation(B)).to(DEV)
        pos = int((perm == at).nonzero()[0, 0])
        for (ts, hl), want in frames.items():
            got = env.render(perm, tile_size=ts, highlight=bool(hl)).cpu().numpy()
            assert (got[pos] == want).all(), (name, cb, ts, hl, int((got[pos] != want).any(axis=2).sum()))
            if ts != 32:
                ref = _composed(spec0, g[perm.cpu().numpy()], a[perm.cpu().numpy()], ts, hl)
                assert (got == ref).all(), (name, cb, ts, hl)


@pytest.mark.parametrize("path", util.RANDSTATE_GOLDEN[:6] + [p for p in util.RANDSTATE_GOLDEN if "64x64" in p],
                         ids=lambda p: p.split("/")[-1][:-4])
def test_frames_of_stepped_random_states(path):
    """Random states of the reference-recorded corpus, stepped on the device with the recorded actions: every env's frame
    equals the composer's over the state the env holds then, in each cell format (16-bit and byte grids)."""
    z, d, spec0 = util.load_golden(path)
    for cb in (2, 3):
        spec = dataclasses.replace(spec0, cell_bytes=cb)
        B = z["grid0"].shape[0]
        env = BatchedMultiGridEnv(spec, B, DEV)
        env.load_state(z["grid0"], z["agents0"], z["rng0"], z["aux"] if spec.env_kind != "empty" else None, z["step_count0"],
                       validate=False)
        for t in range(min(4, z["actions"].shape[0])):
            env.step(torch.from_numpy(z["actions"][t]).to(DEV))
        grid, agents = env.grid.cpu().numpy(), env.agents.cpu().numpy()
        assert (grid == z["grid"][t]).all()
        for ts, hl in ((8, 1), (4, 0), (3, 1)):
            got = env.render(tile_size=ts, highlight=bool(hl)).cpu().numpy()
            assert (got == _composed(spec0, grid, agents, ts, hl)).all(), (path, cb, ts, hl)


def test_largest_grid_frame():
    """255 x 255, view 15, agents on the far edges: 12.5 MB of frame per env at ts 8."""
    z, d, spec = util.load_golden(os.path.join(ru.GOLDEN, "empty255_a3_v15_edges.npz"))
    grid = layouts.grid_to_product(z["grid"][-1])[None]
    agents = layouts.pack_agents(z["agents"][-1])[None]
    env = BatchedMultiGridEnv(spec, 1, DEV)
    env.load_state(grid, agents)
    for hl in (1, 0):
        got = env.render(tile_size=8, highlight=bool(hl)).cpu().numpy()
        assert got.shape == (1, 255 * 8, 255 * 8, 3)
        assert (got == _composed(spec, grid, agents, 8, hl)).all()


def test_render_leaves_state_and_buffers_untouched():
    spec = EnvSpec(16, 16, 4, 7, max_steps=100)
    B = 64
    st = util.random_state(spec, B, seed=5)
    env = BatchedMultiGridEnv(spec, B, DEV)
    env.load_state(st["grid"], st["agents"], st["rng"], st["target"], st["step_count"])
    env.step(torch.from_numpy(util.random_actions(B, 4, seed=1)).to(DEV))
    oh, _ = env.gen_obs(one_hot=True)
    env.step(torch.from_numpy(util.random_actions(B, 4, seed=2)).to(DEV))
    before = {k: getattr(env, k).clone() for k in ("cells", "agents", "rng", "step_count", "aux", "obs", "dir", "reward",
                                                    "terminated", "truncated", "err")}
    out_bytes, oh_bytes = env._out.clone(), oh.clone()
    for kw in (dict(), dict(env_ids=torch.tensor([5, 3, 63], device=DEV), tile_size=8), dict(tile_size=7, highlight=False)):
        env.render(**kw)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(env, k), v), k
    assert torch.equal(env._out, out_bytes) and torch.equal(env._one_hot, oh_bytes)
    env.check_errors()
