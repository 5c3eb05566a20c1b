"""View frames on the MI355X (include/mgx.h "VIEW FRAMES": mgx_render_views, BatchedMultiGridEnv.render_views,
wrappers.RGBImgPartialObsWrapper): the device bytes against the frames the reference's Grid.render drew and against the NumPy
composer (tests/view_frames_util.py) over stepped states and arbitrary bytes, every path of the launcher, offsets past 2^31,
traces, env_ids, no side effects, graph capture and the dict wrapper."""
import numpy as np
import pytest
import torch

import multigrid_amd as mg
from multigrid_amd import BatchedMultiGridEnv, EnvSpec, ops, wrappers
from oracle import binding as ob
from tests import render_util as ru
from tests import util
from tests import view_frames_util as vu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPEC = EnvSpec(12, 10, 5, 7, max_steps=50)            # the spec the recorded views came from


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _draw(obs, dirs, colours, ts, hl, cf=False):
    """mgx_render_views over flat views obs u8[n,v,v,3], dirs / colours u8[n] -> numpy frames."""
    n, v = obs.shape[0], obs.shape[1]
    be = ops.HipBackend(EnvSpec(8, 8, 1, v, max_steps=10), DEV)
    P = v * ts
    frames = torch.empty((n, 3, P, P) if cf else (n, P, P, 3), dtype=torch.uint8, device=DEV)
    be.render_views(n, _dev(obs), _dev(dirs), _dev(colours), ts, bool(hl), bool(cf), frames)
    return frames.cpu().numpy()


def _random_views(seed, B=8, spec=SPEC):
    st = util.random_state(spec, B, seed=seed)
    obs, dirs = ob.gen_obs_batch(spec.as_dict(), st["grid"], st["agents"])
    v = spec.view_size
    return obs.reshape(-1, v, v, 3), dirs.reshape(-1), st["agents"][:, :, 0].reshape(-1).copy()


def _loaded(spec, B, seed, colours=False):
    st = util.random_state(spec, B, seed=seed)
    if colours:                                            # per-env differing agent colours
        st["agents"][:, :, 0] = np.random.default_rng(seed).integers(0, 6, size=st["agents"].shape[:2])
    env = BatchedMultiGridEnv(spec, B, DEV)
    env.load_state(st["grid"], st["agents"], st["rng"], st["target"], st["step_count"])
    return env


def _env_views(env):
    return env.obs.cpu().numpy(), env.dir.cpu().numpy(), env.agents[:, :, 0].cpu().numpy()


def _composed(obs, dirs, colours, ts, hl, cf=False):
    """the composer over views of any leading shape"""
    v = obs.shape[-2]
    flat = vu.compose_views(obs.reshape(-1, v, v, 3), dirs.reshape(-1), colours.reshape(-1), ru.host_atlas(ts), bool(hl), bool(cf))
    return flat.reshape(tuple(dirs.shape) + flat.shape[1:])


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("stores", ("nt", "plain"))
def test_recorded_frames(stores, monkeypatch):
    """The recorded views at random positions among random views: theirs are the reference's bytes, the others the composer's; the
    16-byte path (ts 8, both store kinds) and the byte path (ts 7)."""
    monkeypatch.setenv("MGX_RENDER_STORES", stores)
    image, fdirs, fcolours, frames = vu.fixture()
    obs, dirs, colours = _random_views(seed=21)
    n, K = len(obs) + len(image), len(image)
    at = np.sort(np.random.default_rng(5).choice(n, K, replace=False))
    rest = np.setdiff1d(np.arange(n), at)
    all_obs, all_dirs, all_col = np.zeros((n,) + obs.shape[1:], np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    all_obs[at], all_dirs[at], all_col[at] = image, fdirs, fcolours
    all_obs[rest], all_dirs[rest], all_col[rest] = obs, dirs, colours
    for (ts, hl), want in frames.items():
        got = _draw(all_obs, all_dirs, all_col, ts, hl)
        assert (got[at] == want).all(), (ts, hl, np.nonzero((got[at] != want).any(axis=(1, 2, 3)))[0])
        assert (got == _composed(all_obs, all_dirs, all_col, ts, hl)).all(), (ts, hl)
        got = _draw(all_obs, all_dirs, all_col, ts, hl, cf=True)
        assert (got[at] == want.transpose(0, 3, 1, 2)).all(), (ts, hl, "channels_first")


# ------------------------------------------------------------------------------------------------------------------ 2
STEPPED = util.RANDSTATE_GOLDEN[:3] + [p for p in util.RANDSTATE_GOLDEN if "a16_v9" in p or "_a1_" in p]
CASES = ((8, 1, 0), (8, 0, 1), (4, 0, 0), (4, 1, 1), (7, 1, 0), (7, 0, 1), (1, 0, 1), (1, 1, 0))      # (ts, highlight, channels_first)


def test_frames_of_stepped_states():
    """Reference-recorded random states stepped on the device with the recorded actions: render_views() equals the composer over
    env.obs / env.dir in both store paths, with and without highlight, in both layouts -- and the views hold what the rule is about."""
    assert any("a16_v9" in p for p in STEPPED) and any("_a1_" in p for p in STEPPED) and len(STEPPED) >= 5
    seen = {"other_agents": 0, "unseen": 0, "carried": 0}
    for path in STEPPED:
        z, d, spec = util.load_golden(path)
        B = z["grid0"].shape[0]
        env = BatchedMultiGridEnv(spec, B, DEV)
        env.load_state(z["grid0"], z["agents0"], z["rng0"], z["aux"] if spec.env_kind != "empty" else None, z["step_count0"],
                       validate=False)
        for t in range(min(3, z["actions"].shape[0])):
            env.step(torch.from_numpy(z["actions"][t]).to(DEV))
        obs, dirs, colours = _env_views(env)
        for k, n in vu.census(obs.reshape((-1,) + obs.shape[2:])).items():
            seen[k] += n
        for ts, hl, cf in CASES:
            got = env.render_views(tile_size=ts, highlight=bool(hl), channels_first=bool(cf))
            P = spec.view_size * ts
            assert tuple(got.shape) == (B, spec.num_agents) + ((3, P, P) if cf else (P, P, 3))
            assert (got.cpu().numpy() == _composed(obs, dirs, colours, ts, hl, cf)).all(), (path, ts, hl, cf)
    assert all(seen.values()), f"the stepped states must show other agents, carried objects and unseen cells: {seen}"


# ------------------------------------------------------------------------------------------------------------------ 3
def test_arbitrary_bytes():
    """64 views of uniformly random bytes, dir and colour in 0..255 (the rule takes dir & 3): any bytes are legal input."""
    r = np.random.default_rng(11)
    obs = r.integers(0, 256, size=(64, 7, 7, 3), dtype=np.uint8)
    dirs, colours = r.integers(0, 256, size=64, dtype=np.uint8), r.integers(0, 256, size=64, dtype=np.uint8)
    obs[:8, ..., 0] = 10                                   # (uniform bytes hold few agent cells: eight views full of them)
    for ts, hl, cf in ((8, 1, 0), (8, 0, 1), (7, 1, 1), (3, 0, 0)):
        assert (_draw(obs, dirs, colours, ts, hl, cf) == _composed(obs, dirs, colours, ts, hl, cf)).all(), (ts, hl, cf)


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("n", (1, 3, 257))
def test_view_counts(n):
    """one view, less than a group, whole groups and a short last one (a group is 4 views at v 7, ts 8)"""
    obs, dirs, colours = _random_views(seed=31, B=52)
    obs, dirs, colours = obs[:n], dirs[:n], colours[:n]
    assert len(obs) == n
    for ts, hl, cf in ((8, 1, 0), (8, 1, 1), (7, 1, 0)):
        assert (_draw(obs, dirs, colours, ts, hl, cf) == _composed(obs, dirs, colours, ts, hl, cf)).all(), (n, ts, cf)


def test_misaligned_out_takes_the_byte_path():
    """out= a contiguous view that starts 4 bytes into a larger buffer: no 16-byte stores, the same bytes, nothing outside them"""
    env = _loaded(SPEC, 8, seed=3)
    env.gen_obs()
    want = env.render_views(tile_size=8)
    buf = torch.full((want.numel() + 32,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[4:4 + want.numel()].view(want.shape)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    got = env.render_views(tile_size=8, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, want)
    assert bool((buf[:4] == 0xA5).all()) and bool((buf[4 + want.numel():] == 0xA5).all())
    assert (want.cpu().numpy() == _composed(*_env_views(env), 8, 1)).all()


def test_largest_and_smallest_frames():
    """v = 15 at ts = 64 (one view, 2.76 MB, a workgroup of its own) and v = 3 at ts = 1 (27 bytes a view, 16 views a workgroup)"""
    big = EnvSpec(18, 17, 2, 15, max_steps=20)
    obs, dirs, colours = _random_views(seed=15, B=1, spec=big)
    for cf in (0, 1):
        assert (_draw(obs[:1], dirs[:1], colours[:1], 64, 1, cf) == _composed(obs[:1], dirs[:1], colours[:1], 64, 1, cf)).all(), cf
    small = EnvSpec(8, 8, 3, 3, max_steps=20)
    obs, dirs, colours = _random_views(seed=14, B=13, spec=small)
    assert len(obs) == 39
    for hl, cf in ((1, 0), (0, 1)):
        assert (_draw(obs, dirs, colours, 1, hl, cf) == _composed(obs, dirs, colours, 1, hl, cf)).all(), (hl, cf)


# ------------------------------------------------------------------------------------------------------------------ 5
def test_offsets_past_2_31():
    """One call at the C4 workload's own output size -- 262 144 views, v 7, ts 8: 2.47 GB.  Its last 8 views and the 8 views around
    the 2^31-byte mark equal the same views rendered alone; compared on the device."""
    N, v, ts = 262144, 7, 8
    F = 3 * (v * ts) ** 2
    assert N * F > 2 ** 31
    base_obs, base_dirs, base_col = _random_views(seed=41)
    g = torch.Generator(device=DEV)
    g.manual_seed(9)
    pick = torch.randint(0, len(base_obs), (N,), device=DEV, generator=g)
    obs, dirs, colours = _dev(base_obs)[pick], _dev(base_dirs)[pick], _dev(base_col)[pick]
    be = ops.HipBackend(EnvSpec(8, 8, 1, v, max_steps=10), DEV)
    mark = 2 ** 31 // F
    for cf in (False, True):
        shape = (3, v * ts, v * ts) if cf else (v * ts, v * ts, 3)
        frames = torch.empty((N,) + shape, dtype=torch.uint8, device=DEV)
        be.render_views(N, obs, dirs, colours, ts, True, cf, frames)
        for lo in (N - 8, mark - 4):
            assert lo * F < 2 ** 31 < (lo + 8) * F or lo == N - 8
            alone = torch.empty((8,) + shape, dtype=torch.uint8, device=DEV)
            be.render_views(8, obs[lo:lo + 8], dirs[lo:lo + 8], colours[lo:lo + 8], ts, True, cf, alone)
            assert torch.equal(frames[lo:lo + 8], alone), (cf, lo)
        del frames
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 6
def test_traces_in_one_call():
    """rollout() outputs [T, B, A, ...] in one call equal T per-step calls; with per-env differing agent colours, colors= given
    explicitly equals the default (the [B, A] colours, repeating every B * A views)."""
    B, T = 6, 5
    env = _loaded(SPEC, B, seed=8, colours=True)
    acts = torch.from_numpy(np.stack([util.random_actions(B, SPEC.num_agents, seed=60 + t) for t in range(T)])).to(DEV)
    out = env.rollout(acts)
    col = env.agents[:, :, 0].contiguous()
    assert len(torch.unique(col, dim=0)) > 1, "the envs must differ in their agents' colours"
    for cf in (False, True):
        whole = env.render_views(out["obs"], out["dir"], channels_first=cf)
        assert tuple(whole.shape[:3]) == (T, B, SPEC.num_agents)
        for t in range(T):
            assert torch.equal(whole[t], env.render_views(out["obs"][t], out["dir"][t], channels_first=cf)), (cf, t)
        explicit = env.render_views(out["obs"], out["dir"], colors=col.expand(T, -1, -1).contiguous(), channels_first=cf)
        assert torch.equal(whole, explicit)
    want = _composed(out["obs"].cpu().numpy(), out["dir"].cpu().numpy(), np.broadcast_to(col.cpu().numpy(), (T,) + tuple(col.shape)), 8, 1)
    assert (env.render_views(out["obs"], out["dir"]).cpu().numpy() == want).all()
    with pytest.raises(ValueError):                        # leading dimensions that do not end in [B, A] need colors=
        env.render_views(out["obs"][:, :3].contiguous(), out["dir"][:, :3].contiguous())


# ------------------------------------------------------------------------------------------------------------------ 7
def test_env_ids_draw_restored_envs_without_a_step():
    B = 8
    env = _loaded(SPEC, B, seed=12, colours=True)
    env.step(torch.from_numpy(util.random_actions(B, SPEC.num_agents, seed=1)).to(DEV))
    snap = env.snapshot()
    for t in range(3):
        env.step(torch.from_numpy(util.random_actions(B, SPEC.num_agents, seed=2 + t)).to(DEV))
    ids = torch.tensor([5, 2, 7], dtype=torch.int64, device=DEV)
    env.restore(snap, ids, ids)
    got = env.render_views(env_ids=ids, tile_size=8)
    grid, agents = env.grid.cpu().numpy()[ids.cpu().numpy()], env.agents.cpu().numpy()[ids.cpu().numpy()]
    obs, dirs = ob.gen_obs_batch(SPEC.as_dict(), np.ascontiguousarray(grid), np.ascontiguousarray(agents))
    assert (got.cpu().numpy() == _composed(obs, dirs, agents[:, :, 0], 8, 1)).all()
    assert not (obs == env.obs.cpu().numpy()[ids.cpu().numpy()]).all(), "the env's own outputs are those of the later steps"
    for bad in (ids.to(torch.int32), ids[None], ids.cpu(), [5, 2], ids.to(torch.float32)):
        with pytest.raises(ValueError):
            env.render_views(env_ids=bad)
    with pytest.raises(ValueError):
        env.render_views(env.obs, env.dir, env_ids=ids)
    env.check_errors()


# ------------------------------------------------------------------------------------------------------------------ 8
def test_render_views_leaves_state_and_buffers_untouched():
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
    trace_obs, trace_dir = env.obs.clone()[None].repeat(2, 1, 1, 1, 1, 1), env.dir.clone()[None].repeat(2, 1, 1)
    given = (trace_obs.clone(), trace_dir.clone())
    for args, kw in (((), dict()), ((), dict(env_ids=torch.tensor([5, 3, 63], device=DEV), tile_size=4, channels_first=True)),
                     ((trace_obs, trace_dir), dict(tile_size=7, highlight=False))):
        env.render_views(*args, **kw)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(env, k), v), k
    assert torch.equal(env._out, out_bytes) and torch.equal(env._one_hot, oh_bytes)
    assert torch.equal(trace_obs, given[0]) and torch.equal(trace_dir, given[1])
    env.check_errors()


# ------------------------------------------------------------------------------------------------------------------ 9
def test_graph_capture_of_step_and_render_views():
    """A step followed by render_views(out=buf) in one graph, replayed with three different action tensors: each replay equals the
    eager result of a twin env."""
    spec, B = EnvSpec(16, 16, 4, 7, max_steps=100), 64
    env, twin = _loaded(spec, B, seed=6), _loaded(spec, B, seed=6)
    acts = [torch.from_numpy(util.random_actions(B, 4, seed=70 + k)).to(DEV) for k in range(4)]
    a = acts[0].clone()
    dev = torch.device(DEV)
    cur, side, graph = torch.cuda.current_stream(dev), torch.cuda.Stream(dev), torch.cuda.CUDAGraph()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        env.step(a)                                       # (everything bound, the atlas made and the buffer allocated before the capture)
        buf = env.render_views(channels_first=True)
        with torch.cuda.graph(graph, stream=side):
            env.step(a)
            env.render_views(channels_first=True, out=buf)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    twin.step(acts[0])                                    # the warm-up step (the capture itself runs nothing)
    assert torch.equal(env.agents, twin.agents) and torch.equal(env.step_count, twin.step_count)
    for k in (1, 2, 3):
        a.copy_(acts[k])
        buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        twin.step(acts[k])
        assert torch.equal(env.obs, twin.obs)
        assert torch.equal(buf, twin.render_views(channels_first=True)), k
    env.check_errors()


# ------------------------------------------------------------------------------------------------------------------ 10
def test_rgb_img_partial_obs_wrapper():
    env = mg.make("MultiGrid-Empty-8x8-v0", agents=2, device=DEV)
    w = wrappers.RGBImgPartialObsWrapper(env, tile_size=8)
    v = env.agents[0].view_size
    P = v * 8

    def want():
        b = env.unwrapped._benv
        return _composed(b.obs.cpu().numpy(), b.dir.cpu().numpy(), b.agents[:, :, 0].cpu().numpy(), 8, 1)[0]

    for agent in env.agents:
        space = agent.observation_space["image"]
        assert tuple(space.shape) == (P, P, 3) and space.dtype == np.uint8
    obs, info = w.reset(seed=4)
    frames = want()
    for i in (0, 1):
        assert obs[i]["image"].dtype == np.uint8 and obs[i]["image"].shape == (P, P, 3)
        assert (obs[i]["image"] == frames[i]).all() and "direction" in obs[i]
    for action in (2, 1, 2):
        obs, reward, terminated, truncated, info = w.step({0: action, 1: 0})
        frames = want()
        for i in (0, 1):
            assert obs[i]["image"].dtype == np.uint8 and (obs[i]["image"] == frames[i]).all()
    assert frames.any() and not (frames[0] == frames[1]).all()
