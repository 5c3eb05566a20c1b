"""Frame rendering on the CPU (no GPU): the g++ build of multigrid_amd/csrc/mgx_render.h -- what the atlas kernel evaluates per
pixel -- against the tiles recorded from the reference (tests/golden/render/, tools/gen_render_golden.py); a NumPy
composer over that atlas and the oracle's gen_obs against the recorded frames; the drop-in env's get_frame / render() on the
oracle backend; the argument checks of the C ABI and of BatchedMultiGridEnv.render."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import multigrid_amd as mg
from multigrid_amd import _lib
from oracle import binding as ob
from tests import render_util as ru
from tests import util


@pytest.mark.parametrize("ts", ru.TILE_SIZES)
def test_host_atlas_matches_every_recorded_tile(ts):
    tiles, overlays, enc = ru.tile_fixture(ts)
    atlas = ru.host_atlas(ts)
    app = ru.appearance(enc[:, 0], enc[:, 1], enc[:, 2])
    bad = []
    for k, ov in enumerate(overlays):
        for hl in (0, 1):
            got = atlas[(app * 25 + ov) * 2 + hl]
            diff = (got != tiles[:, k, hl]).any(axis=(1, 2, 3))
            bad += [(tuple(enc[e]), int(ov), hl) for e in np.nonzero(diff)[0]]
    assert not bad, f"{len(bad)} tiles differ at ts={ts}, e.g. {bad[:8]}"


def test_key_space_has_fifty_appearances():
    """162 encodings draw 50 distinct tiles at ts 8 (goal = wall of its colour, every empty and lava alike), and the appearance
    index tells them apart exactly."""
    tiles, _, enc = ru.tile_fixture(8)
    app = ru.appearance(enc[:, 0], enc[:, 1], enc[:, 2])
    assert len(set(app.tolist())) == 50
    for a in set(app.tolist()):
        same = np.nonzero(app == a)[0]
        assert all((tiles[e] == tiles[same[0]]).all() for e in same)
    distinct = {tiles[e, 0, 0].tobytes() for e in range(len(enc))}
    assert len(distinct) == 50
    lib = ru.shim()
    for t in range(16):
        for c in range(8):
            for s in range(4):
                assert lib.shim_render_appearance(t, c, s) == int(ru.appearance(t, c, s)), (t, c, s)


def test_rotation_constants_come_from_libm():
    c, s = np.zeros(4), np.zeros(4)
    ru.shim().shim_render_trig(c.ctypes.data, s.ctypes.data)
    for d in range(4):
        theta = 0.5 * np.pi * d
        assert c[d] == math.cos(-theta) and s[d] == math.sin(-theta), d


@pytest.mark.parametrize("name", [f[0] for f in ru.frame_fixtures()])
def test_composer_matches_recorded_frames(name):
    (_, spec, grid, agents, frames), = [f for f in ru.frame_fixtures() if f[0] == name]
    obs, _ = ob.gen_obs_batch(spec.as_dict(), grid[None], agents[None])
    for (ts, hl), want in frames.items():
        got = ru.compose(spec, grid, agents, obs[0] if hl else None, ru.host_atlas(ts))
        assert got.shape == want.shape and (got == want).all(), (name, ts, hl, int((got != want).any(axis=2).sum()))


class RenderOracleBackend(util.OracleBackend):
    """The oracle backend plus `render`, composed on the host from the g++ atlas."""

    def render(self, n, grid, agents, obs, tile_size, frames):
        g3 = self._g3(grid)
        for b in range(n):
            o = obs[b].numpy() if obs is not None else None
            frames[b].copy_(torch.from_numpy(ru.compose(self.spec, g3[b], agents[b].numpy(), o, ru.host_atlas(tile_size))))


def _dropin(spec, grid, agents, **kw):
    env = mg.MultiGridEnv(width=spec.width, height=spec.height, agents=spec.num_agents, agent_view_size=spec.view_size,
                          see_through_walls=spec.see_through_walls, device="cpu", _backend=RenderOracleBackend, **kw)
    env._benv.load_state(grid[None], agents[None])
    return env


@pytest.mark.parametrize("name", ["empty_a2", "stacked_agents", "playground", "see_through_walls"])
def test_dropin_get_frame_and_render_match_recorded_frames(name):
    (_, spec, grid, agents, frames), = [f for f in ru.frame_fixtures() if f[0] == name]
    env = _dropin(spec, grid, agents)
    for (ts, hl), want in frames.items():
        got = env.get_frame(highlight=bool(hl), tile_size=ts)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and (got == want).all(), (name, ts, hl)
        assert (env.get_full_render(bool(hl), ts) == want).all()
    env = _dropin(spec, grid, agents, render_mode="rgb_array", highlight=False, tile_size=7)
    assert env.render_mode == "rgb_array" and "rgb_array" in env.metadata["render_modes"]
    assert (env.render() == frames[7, 0]).all()
    env = _dropin(spec, grid, agents, render_mode="rgb_array")
    assert env.highlight and env.tile_size == 32
    if (32, 1) in frames:
        assert (env.render() == frames[32, 1]).all()


def test_render_modes_that_stay_refused():
    spec = mg.EnvSpec(8, 8, 2, 7, max_steps=10)
    grid, agents = (ru.frame_fixtures()[0][2], ru.frame_fixtures()[0][3])
    env = _dropin(spec, grid, agents)
    with pytest.raises(NotImplementedError):
        env.render()                                       # render_mode=None: still refused (tests/test_env_compat.py)
    with pytest.raises(NotImplementedError):
        env.get_pov_render()
    with pytest.raises(NotImplementedError):
        env.get_frame(agent_pov=True)
    with pytest.raises(NotImplementedError):
        mg.MultiGridEnv(width=8, height=8, agents=2, render_mode="human", device="cpu", _backend=RenderOracleBackend)
    assert _lib.ABI_VERSION == 11 and _lib.lib().mgx_abi_version() == 11
    assert "mgx_render" in _lib.EXPORTS and "mgx_render_atlas" in _lib.EXPORTS


def test_batched_render_argument_checks():
    (_, spec, grid, agents, frames), = [f for f in ru.frame_fixtures() if f[0] == "stacked_agents"]
    B = 5
    env = mg.BatchedMultiGridEnv(spec, B, "cpu", backend=RenderOracleBackend(spec))
    env.load_state(np.repeat(grid[None], B, 0), np.repeat(agents[None], B, 0))
    for ts in (0, 65, -1):
        with pytest.raises(ValueError):
            env.render(tile_size=ts)
    with pytest.raises(ValueError):
        env.render(torch.tensor([0, B]), tile_size=8)
    with pytest.raises(ValueError):
        env.render(torch.tensor([-1]), tile_size=8)
    with pytest.raises(ValueError):
        env.render(torch.tensor([[0, 1]]), tile_size=8)
    with pytest.raises(TypeError):
        env.render(torch.tensor([0.0, 1.0]), tile_size=8)
    with pytest.raises(ValueError):
        env.render(tile_size=8, out=torch.zeros((B, 8, 8, 3), dtype=torch.uint8))
    got = env.render(torch.tensor([3, 1]), tile_size=8)
    assert got.shape == (2, spec.height * 8, spec.width * 8, 3)
    assert (got[0].numpy() == frames[8, 1]).all() and (got[1].numpy() == frames[8, 1]).all()
    out = torch.zeros((B, spec.height * 7, spec.width * 7, 3), dtype=torch.uint8)
    assert env.render(tile_size=7, highlight=False, out=out) is out and (out[4].numpy() == frames[7, 0]).all()
    assert env.render(torch.zeros(0, dtype=torch.long), tile_size=8).shape == (0, spec.height * 8, spec.width * 8, 3)


def test_c_abi_refuses_bad_arguments():
    """mgx_render / mgx_render_atlas check their arguments before touching the device."""
    L = _lib.lib()
    spec = mg.EnvSpec(8, 8, 2, 7, max_steps=10)
    sc = spec.to_c()
    dummy = C.c_void_p(16)
    for ts in (0, 65, -3):
        assert L.mgx_render_atlas(ts, dummy, None) == _lib.ERR_INVALID_ARGUMENT
        assert L.mgx_render(C.byref(sc), 1, dummy, dummy, None, dummy, ts, dummy, None) == _lib.ERR_INVALID_ARGUMENT
    assert L.mgx_render_atlas(8, None, None) == _lib.ERR_INVALID_ARGUMENT
    for k in range(4):
        ptrs = [dummy] * 4
        ptrs[k] = None
        g, a, atlas, frames = ptrs
        assert L.mgx_render(C.byref(sc), 1, g, a, None, atlas, 8, frames, None) == _lib.ERR_INVALID_ARGUMENT
    assert L.mgx_render(C.byref(sc), -1, dummy, dummy, None, dummy, 8, dummy, None) == _lib.ERR_INVALID_ARGUMENT
    assert L.mgx_render(C.byref(sc), 0, None, None, None, None, 8, None, None) == _lib.OK
    assert L.mgx_render(None, 1, dummy, dummy, None, dummy, 8, dummy, None) == _lib.ERR_INVALID_ARGUMENT


def test_render_goldens_stay_small():
    import os
    total = sum(os.path.getsize(os.path.join(ru.RENDER_GOLDEN, f)) for f in os.listdir(ru.RENDER_GOLDEN))
    assert total <= 1 << 20, total
    names = [f[0] for f in ru.frame_fixtures()]
    assert len(names) >= 12
