"""BatchedMultiGridEnv.reset(seed, mask) -- restarts of the envs the CALLER chooses -- on the CPU: the host logic over an oracle
launcher that builds the two new backend calls (reset_select / reset_generate_select) from the existing DONE-based oracle resets.

Truth: the unseeded reset corpus (tests/golden/resets_*.npz), the seeded resets of the real reference recorded by
tools/record_seeded_resets.py (tests/golden/seeded/seeded_resets.npz), and multigrid_amd/layouts.py on numpy's own
Generator(PCG64(SeedSequence([seed, g]))) for the other global indices.  The helpers are shared with tests/test_reset_select_gpu.py,
which holds the kernels to this oracle-backed env and to the recorded bytes."""
import ctypes as C
import dataclasses
import json
import os
import types

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib, layouts, rng as rnglib
from multigrid_amd.sharding import NodeEnv
from tests import util
from tests.test_reference_resets import check_state, inject, layouts_py, load, make_env, recorded_aux

SEEDED_PATH = os.path.join(util.GOLDEN_DIR, "seeded", "seeded_resets.npz")
SEEDED_TAGS = ("empty_fixed_5_a3", "empty_random_6_a3", "bup_rs5_a2", "rbd_5_a2", "lh_2rooms_rs5_k33_a2", "playground_1x1_rs7_a1")
STATE = ("cells", "agents", "aux", "rng", "step_count", "episode")


class SelectOracle(util.OracleBackend):
    """util.OracleBackend + the two selected restarts, made of its done-based ones: the chosen envs are marked finished, the done
    state of the others is hidden, the done-based reset runs, and the others get their agent rows and step counts back."""

    def _selected(self, B, select):
        return np.ones(B, bool) if select is None else select.numpy().astype(bool)

    def _as_done(self, sel, agents, step_count, call):
        keep = torch.from_numpy(~sel)
        rows, counts = agents.clone(), step_count.clone()
        step_count[torch.from_numpy(sel)] = self.spec.max_steps
        step_count[keep] = 0
        agents[keep, :, 4] = 0
        call()
        agents[keep] = rows[keep]
        step_count[keep] = counts[keep]

    def reset_generate_select(self, B, gen, select, rng_words, grid, agents, rng, step_count, aux, episode, was_reset):
        sel = self._selected(B, select)
        if rng_words is not None:                       # a fresh generator: its words, no pending 32-bit half
            rng[torch.from_numpy(sel)] = rng_words[torch.from_numpy(sel)]
            gen["gen_state"][torch.from_numpy(sel), 5] = 0
        self._as_done(sel, agents, step_count,
                      lambda: self.reset_generate(B, gen, grid, agents, rng, step_count, aux, episode, was_reset))

    def reset_select(self, B, first_env, pool, select, rng_words, grid, agents, rng, step_count, target, episode, was_reset):
        sel = self._selected(B, select)
        if rng_words is not None:
            rng[torch.from_numpy(sel)] = rng_words[torch.from_numpy(sel)]
        self._as_done(sel, agents, step_count,
                      lambda: self.reset_done(B, first_env, pool, grid, agents, step_count, target, episode, was_reset))


class Seeded:
    """One generator kind of seeded_resets.npz with the interface of a resets_*.npz file (z[key], z.files)."""

    def __init__(self, tag):
        z = np.load(SEEDED_PATH)
        self._d = {k[len(tag) + 1:]: z[k] for k in z.files if k.startswith(tag + ".")}
        self.files = list(self._d)
        self.d = json.loads(str(self._d["spec_json"]))
        self.spec, self.gen = EnvSpec.from_dict(self.d), self.d["gen"]

    def __getitem__(self, k):
        return self._d[k]


def snapshot(env):
    out = {k: getattr(env, k).cpu().clone() for k in STATE}
    if getattr(env, "_gen", None) is not None:
        out["gen_state"] = env._gen["gen_state"].cpu().clone()
    return out


def assert_unchanged(env, before, keep, ctx):
    """the envs of `keep` (bool[B]) hold the bytes of `before`"""
    keep = torch.as_tensor(keep)
    for k, v in snapshot(env).items():
        assert torch.equal(v[keep], before[k][keep]), f"{ctx}: {k} of an env that was not selected changed"


def sub_env(env, idx):
    """the envs `idx` of `env` as an object check_state() can read"""
    idx = torch.as_tensor(idx, device=env.cells.device)
    v = types.SimpleNamespace(spec=env.spec, grid=env.grid[idx], _gen={"gen_state": env._gen["gen_state"][idx]})
    for k in ("agents", "aux", "rng", "step_count", "episode", "was_reset"):
        setattr(v, k, getattr(env, k)[idx])
    return v


def live_env(z, spec, gen, idx, dev, done_at=(), **kw):
    """make_env's batch (env b = recorded event idx[b], generators injected) with every episode RUNNING -- one step in -- but the envs
    `done_at`, which stay finished"""
    env = make_env(z, spec, gen, idx, dev, **kw)
    env.step_count.fill_(1)
    for b in done_at:
        env.step_count[b] = spec.max_steps
    return env


def seeded_generator(seed, g):
    """np_random of global env g after reset(seed): the rule BatchedMultiGridEnv.seed() documents, on numpy itself"""
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed if g == 0 else [seed, g])))


def expected_seeded(z, spec, gen, event, seed, g):
    """layouts.py on the recorded placement state of `event` and the fresh np_random of (seed, g) -> grid, agents, aux, rng5, lay5"""
    lay, npr = rnglib.generator_from_gen_words(z["lay_before"][event]), seeded_generator(seed, g)
    grid, agents, target = layouts_py(spec, gen, lay, npr)
    aux = np.zeros(16, np.uint8)
    if spec.env_kind != "empty":
        aux = layouts.make_aux(spec.env_kind, grid, target=target)
    return grid, agents, aux, rnglib.gen_words_from_generator(npr), rnglib.gen_words_from_generator(lay)


def check_seeded(env, z, gen, idx, seed, envs, ctx):
    """the envs `envs` of `env` (env b = event idx[b]) after reset(seed) == layouts.py on the numpy generators of their global index"""
    gs = env._gen["gen_state"].cpu().numpy().view(np.uint64)
    grid, agents, aux, rng = env.grid.cpu().numpy(), env.agents.cpu().numpy(), env.aux.cpu().numpy(), env.rng.cpu().numpy().view(np.uint64)
    for b in envs:
        g, a, x, npr5, lay5 = expected_seeded(z, env.spec, gen, int(idx[b]), seed, env.first_env + int(b))
        c = f"{ctx} env {b} (global {env.first_env + int(b)})"
        np.testing.assert_array_equal(grid[b], g, err_msg=c + ": grid")
        np.testing.assert_array_equal(agents[b], a, err_msg=c + ": agents")
        if env.spec.env_kind != "empty":
            np.testing.assert_array_equal(aux[b], x, err_msg=c + ": aux")
        np.testing.assert_array_equal(rng[b], npr5[:4], err_msg=c + ": rng")
        np.testing.assert_array_equal(gs[b, :5], lay5, err_msg=c + ": gen_state[:5]")
        assert gs[b, 5] == npr5[4], c + ": gen_state[5]"


def alternating(B, dev="cpu", dtype=torch.bool):
    return (torch.arange(B, device=dev) % 2 == 0).to(dtype)


# ---- unseeded: the reset corpus --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", util.RESETS_IDS)
def test_unseeded_selected_resets_reproduce_the_corpus(name):
    z, d, spec, gen = load(name)
    E = len(z["lay_before"])
    idx = np.arange(E)
    env = live_env(z, spec, gen, idx, "cpu", done_at=(1,), backend=SelectOracle(spec))
    assert not bool(env.is_done()[0]) and bool(env.is_done()[1])
    mask = alternating(E)
    before = snapshot(env)
    obs, dirs = env.reset(mask=mask)
    sel = mask.nonzero().flatten().numpy()
    check_state(sub_env(env, sel), z, gen, idx[sel], name)
    np.testing.assert_array_equal(obs.numpy()[sel], z["obs0"][idx[sel]])
    assert_unchanged(env, before, ~mask, name)
    assert torch.equal(env.was_reset, mask.to(torch.uint8))
    assert bool(env.is_done()[1]), "a finished env that was not selected stays finished"


# ---- seeded: the reference's own reset(seed=s), then the other global indices -------------------------------------------------------

@pytest.mark.parametrize("tag", SEEDED_TAGS)
def test_seeded_reset_of_env_0_is_the_references(tag):
    z = Seeded(tag)
    assert (z["npr_before"][:, 4] >> np.uint64(32)).any(), "the fixture holds no pending np_random half to drop"
    for n, seed in enumerate(z["seed"].tolist()):
        env = live_env(z, z.spec, z.gen, np.array([n]), "cpu", backend=SelectOracle(z.spec))
        assert int(env._gen["gen_state"][0, 5]) == int(z["npr_before"][n, 4].view(np.int64))
        obs, _ = env.reset(seed=seed)
        check_state(env, z, z.gen, np.array([n]), f"{tag} seed {seed}")
        np.testing.assert_array_equal(obs.numpy(), z["obs0"][n:n + 1])
        # ... and the recorded bytes are what layouts.py makes of numpy's SeedSequence(seed)
        check_seeded(env, z, z.gen, np.array([n]), seed, [0], tag)


@pytest.mark.parametrize("tag,first_env", [("bup_rs5_a2", 0), ("bup_rs5_a2", 5), ("playground_1x1_rs7_a1", 2), ("empty_random_6_a3", 1)])
def test_seeded_reset_follows_the_global_env_index(tag, first_env):
    z = Seeded(tag)
    idx = np.array([0, 1, 2, 3, 0, 1])
    env = live_env(z, z.spec, z.gen, idx, "cpu", backend=SelectOracle(z.spec), first_env=first_env)
    mask = alternating(len(idx), dtype=torch.uint8)
    before = snapshot(env)
    env.reset(seed=11, mask=mask)
    check_seeded(env, z, z.gen, idx, 11, mask.nonzero().flatten().tolist(), f"{tag} first_env={first_env}")
    assert_unchanged(env, before, mask == 0, tag)
    words = rnglib.words_from_seed_and_index(11, first_env + np.arange(len(idx)))
    for b in range(len(idx)):                            # (the host's words ARE numpy's)
        np.testing.assert_array_equal(words[b], rnglib.gen_words_from_generator(seeded_generator(11, first_env + b))[:4])


def test_sharded_reset_equals_one_env_over_the_global_batch():
    z = Seeded("bup_rs5_a2")
    spec, gen, B = z.spec, z.gen, 7

    def setup(e):
        g0, a0, t0 = layouts.blockedunlockpickup_layout(gen["room_size"], spec.num_agents, np.random.default_rng(1), np.random.default_rng(2))
        e.load_state(g0, a0, aux=layouts.make_aux("blockedunlockpickup", g0, target=t0))
        e.set_layout_generator("blockedunlockpickup", layout_seed=3, room_size=gen["room_size"], staged=False)
        e.seed(4)

    one = BatchedMultiGridEnv(spec, B, "cpu", backend=SelectOracle(spec))
    node = NodeEnv(spec, B, ["cpu", "cpu"], backend_factory=lambda sp, dev: SelectOracle(sp))
    setup(one); setup(node)
    mask = alternating(B)
    for kw in (dict(seed=9, mask=mask), dict(mask=~mask), dict(seed=2)):
        obs, _ = one.reset(**kw)
        outs = node.reset(**kw)
        assert torch.equal(torch.cat([o[0] for o in outs]), obs)
        for k in STATE + ("was_reset",):
            assert torch.equal(node.gather(k), getattr(one, k)), k
        assert torch.equal(torch.cat([sh._gen["gen_state"] for sh in node.shards]), one._gen["gen_state"])
    # the first episode of a fresh node: nothing loaded, reset(seed) of everything
    one = BatchedMultiGridEnv(spec, B, "cpu", backend=SelectOracle(spec))
    node = NodeEnv(spec, B, ["cpu", "cpu"], backend_factory=lambda sp, dev: SelectOracle(sp))
    for e in (one, node):
        e.set_layout_generator("blockedunlockpickup", layout_seed=3, room_size=gen["room_size"], staged=False)
    obs, _ = one.reset(seed=5)
    assert torch.equal(torch.cat([o[0] for o in node.reset(seed=5)]), obs)
    for k in STATE:
        assert torch.equal(node.gather(k), getattr(one, k)), k


# ---- the pool form -----------------------------------------------------------------------------------------------------------------

def pool_env(spec, B, dev, first_env, K=5, seed=3, **kw):
    """A running batch over a pool of K layouts; the episode counters differ per env"""
    hooks = spec.env_kind != "empty"
    st = util.random_state(spec, B, seed, terminated_p=0.0, carry_p=0.0)
    pool = util.random_state(spec, K, seed + 1, terminated_p=0.0, density=0.3, carry_p=0.0)
    env = BatchedMultiGridEnv(spec, B, dev, first_env=first_env, **kw)
    env.load_state(st["grid"], st["agents"], st["rng"], st["target"] if hooks else None, np.minimum(st["step_count"], spec.max_steps - 1))
    env.set_layout_pool(pool["grid"], pool["agents"], pool["target"] if hooks else None)
    env.episode.copy_(torch.from_numpy((np.arange(B) * 5 % 7).astype(np.int32)))
    return env, pool


def check_pool(env, pool, before, mask, seed, ctx):
    """selected envs hold their pool layout (index from the GLOBAL env index and the episode BEFORE), the others their old bytes"""
    sp, B = env.spec, env.batch
    sel = np.ones(B, bool) if mask is None else mask.cpu().numpy().astype(bool)
    K = len(pool["grid"])
    lay = (env.first_env + np.arange(B) + before["episode"].numpy().astype(np.int64) * 7919) % K
    cells = torch.from_numpy(layouts.pack_cells_for(sp, pool["grid"]))
    got = snapshot(env)
    s = torch.from_numpy(sel)
    assert torch.equal(got["cells"][s], cells[lay[sel]].view(got["cells"].dtype)), ctx + ": cells"
    assert torch.equal(got["agents"][s], torch.from_numpy(pool["agents"][lay[sel]])), ctx + ": agents"
    if sp.env_kind != "empty":
        assert torch.equal(got["aux"][s], torch.from_numpy(pool["target"][lay[sel]])), ctx + ": aux"
    assert torch.equal(got["episode"][s], before["episode"][s] + 1) and not bool(got["step_count"][s].any()), ctx
    if seed is None:
        assert torch.equal(got["rng"], before["rng"]), ctx + ": an unseeded restart leaves np_random running"
    else:
        words = rnglib.words_from_seed_and_index(seed, env.first_env + np.arange(B)).view(np.int64)
        assert torch.equal(got["rng"][s], torch.from_numpy(words)[s]), ctx + ": rng"
    assert_unchanged(env, before, ~s, ctx)
    assert torch.equal(env.was_reset.cpu(), s.to(torch.uint8)), ctx + ": was_reset"


POOL_SPECS = {"empty8_a1_c2": EnvSpec(8, 8, 1, 7, max_steps=20), "9x7_a3_c3": EnvSpec(9, 7, 3, 5, max_steps=20, cell_bytes=3),
              "empty8_a2_c1": EnvSpec(8, 8, 2, 7, max_steps=20, cell_bytes=1),
              "bup_11x6_a2": EnvSpec(11, 6, 2, 7, max_steps=20, joint_reward=True, env_kind="blockedunlockpickup")}


@pytest.mark.parametrize("seed", [None, 6], ids=["unseeded", "seeded"])
@pytest.mark.parametrize("name", list(POOL_SPECS))
def test_pool_restarts_of_selected_envs(name, seed):
    spec = POOL_SPECS[name]
    B = 9
    for mask in (alternating(B), alternating(B, dtype=torch.uint8) ^ 1, None):
        env, pool = pool_env(spec, B, "cpu", first_env=4, backend=SelectOracle(spec))
        before = snapshot(env)
        obs, _ = env.reset(seed=seed, mask=mask)
        check_pool(env, pool, before, mask, seed, f"{name} seed={seed}")
        ref = BatchedMultiGridEnv(spec, B, "cpu", backend=SelectOracle(spec))
        ref.load_state(env.grid, env.agents, aux=env.aux)
        assert torch.equal(obs, ref.gen_obs()[0]), "reset() returns gen_obs() of the whole batch"


def test_an_all_zero_mask_changes_nothing():
    z, d, spec, gen = load("resets_bup_rs5_a2")
    E = len(z["lay_before"])
    env = live_env(z, spec, gen, np.arange(E), "cpu", done_at=(2,), backend=SelectOracle(spec))
    before = snapshot(env)
    env.was_reset.fill_(1)
    env.reset(seed=3, mask=torch.zeros(E, dtype=torch.bool))
    assert_unchanged(env, before, np.ones(E, bool), "all-zero mask")
    assert not bool(env.was_reset.any())
    env, pool = pool_env(POOL_SPECS["bup_11x6_a2"], 6, "cpu", 0, backend=SelectOracle(POOL_SPECS["bup_11x6_a2"]))
    before = snapshot(env)
    env.reset(seed=3, mask=torch.zeros(6, dtype=torch.uint8))
    assert_unchanged(env, before, np.ones(6, bool), "all-zero mask, pool")


# ---- errors --------------------------------------------------------------------------------------------------------------------------

def test_reset_refuses_what_it_cannot_do():
    spec = EnvSpec(8, 8, 2, 7, max_steps=20)
    mk = lambda: BatchedMultiGridEnv(spec, 4, "cpu", backend=SelectOracle(spec))
    env = mk()
    with pytest.raises(RuntimeError, match="set_layout_pool\\(\\) or set_layout_generator\\(\\)"):
        env.reset(seed=1)
    env.set_layout_generator("empty_random", layout_seed=1, staged=False)
    with pytest.raises(RuntimeError, match="no state loaded"):                 # nothing loaded: only the whole batch can start
        env.reset(seed=1, mask=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="never been seeded"):
        env.reset()
    assert not env._loaded
    for seeded in (lambda e: e.seed(1), lambda e: e.seed_synthetic(1)):            # a seeded batch may start unseeded
        e = mk(); e.set_layout_generator("empty_random", layout_seed=1, staged=False); seeded(e)
        e.reset()
        assert e._loaded and int(e.episode.sum()) == 4 and bool(e.was_reset.all())
    env.reset(seed=1)                                                             # the first episode
    assert env._loaded and bool(env.was_reset.all()) and not bool(env.step_count.any())
    env.reset()                                                                   # ... and reset(seed) itself counts as seeding
    for bad in (torch.ones(3, dtype=torch.bool), torch.ones((4, 1), dtype=torch.bool), torch.ones(4, dtype=torch.int32),
                torch.ones(4, dtype=torch.float32), torch.ones(4, dtype=torch.bool, device="meta"), [1, 0, 1, 0],
                torch.ones(8, dtype=torch.bool)[::2]):
        with pytest.raises(ValueError, match="mask must be"):
            env.reset(mask=bad)
    env._session = object()
    with pytest.raises(RuntimeError, match="persistent session"):
        env.reset()
    env._session = None
    st = util.random_state(spec, 4, 1)
    e = mk(); e.set_layout_generator("empty_random", layout_seed=1, staged=False)
    e.load_state(st["grid"], st["agents"], st["rng"])                             # load_state(rng=...) counts as seeding too
    e.reset(mask=torch.ones(4, dtype=torch.bool))


def test_c_abi_argument_validation():
    L = _lib.lib()
    INV, UNS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
    p = 4096                                                                      # (never dereferenced: every call returns before a launch)
    sel = _lib.MgxResetSelect(None, None)
    spec = EnvSpec(9, 5, 2, 5, max_steps=9, joint_reward=True, env_kind="blockedunlockpickup")
    sc = spec.to_c()
    gen = _lib.MgxLayoutGen(_lib.GEN_KINDS["blockedunlockpickup"], 5, 1, 1, 0, 1, 2, p, p)
    G = lambda sc_, B, s, g, *ptrs: L.mgx_reset_generate_select(C.byref(sc_) if sc_ else None, B, C.byref(s) if s else None,
                                                                 C.byref(g) if g else None, *ptrs, None)
    ok = (p, p, p, p, p, p, None)                       # grid, agents, rng, step_count, aux, episode, was_reset
    assert G(None, 4, sel, gen, *ok) == INV and G(sc, 4, None, gen, *ok) == INV and G(sc, 4, sel, None, *ok) == INV
    assert G(sc, -1, sel, gen, *ok) == INV
    assert G(sc, 0, sel, gen, *ok) == 0 and G(sc, 0, sel, gen, None, None, None, None, None, None, None) == 0      # batch 0: a no-op
    for k in (0, 1, 2, 3, 5):                                                     # a NULL state pointer
        assert G(sc, 4, sel, gen, *[None if i == k else v for i, v in enumerate(ok)]) == INV, k
    assert G(sc, 4, sel, gen, p, p, p, p, None, p, None) == INV                  # a hook env needs aux
    assert G(sc, 4, _lib.MgxResetSelect(p, p + 4), gen, *ok) == INV              # rng_words: 8-byte aligned
    assert G(sc, 4, sel, gen, p, p, p + 4, p, p, p, None) == INV
    # spec checks come before pointer checks
    assert G(dataclasses.replace(spec, cell_bytes=1).to_c(), 4, sel, gen, None, None, None, None, None, None, None) == UNS
    assert G(EnvSpec(255, 5, 2, 5, max_steps=9).to_c(), 4, sel, gen, None, None, None, None, None, None, None) == UNS
    assert G(EnvSpec(7, 4, 3, 3, max_steps=9, joint_reward=True, env_kind="blockedunlockpickup").to_c(), 4, sel,
             _lib.MgxLayoutGen(_lib.GEN_KINDS["blockedunlockpickup"], 4, 1, 1, 0, 1, 2, p, p), *ok) == UNS            # check_layout_gen
    assert G(sc, 4, sel, _lib.MgxLayoutGen(9, 5, 1, 1, 0, 1, 2, p, p), *ok) == UNS                                     # no such generator
    pool = _lib.MgxAutoReset(0, 3, p, p, p, p, None)
    P = lambda sc_, B, s, a, *ptrs: L.mgx_reset_select(C.byref(sc_) if sc_ else None, B, C.byref(s) if s else None,
                                                        C.byref(a) if a else None, *ptrs, None)
    okp = (p, p, p, p, p)                               # grid, agents, rng, step_count, aux
    assert P(None, 4, sel, pool, *okp) == INV and P(sc, 4, None, pool, *okp) == INV and P(sc, 4, sel, None, *okp) == INV
    assert P(sc, -1, sel, pool, *okp) == INV
    assert P(sc, 4, sel, _lib.MgxAutoReset(0, 0, p, p, p, p, None), *okp) == INV and P(sc, 4, sel, _lib.MgxAutoReset(-1, 3, p, p, p, p, None), *okp) == INV
    assert P(sc, 0, sel, pool, *okp) == 0 and P(sc, 0, sel, pool, None, None, None, None, None) == 0
    for k in (0, 1, 3):
        assert P(sc, 4, sel, pool, *[None if i == k else v for i, v in enumerate(okp)]) == INV, k
    for bad in (_lib.MgxAutoReset(0, 3, None, p, p, p, None), _lib.MgxAutoReset(0, 3, p, None, p, p, None), _lib.MgxAutoReset(0, 3, p, p, p, None, None)):
        assert P(sc, 4, sel, bad, *okp) == INV
    assert P(sc, 4, _lib.MgxResetSelect(None, p), pool, p, p, None, p, p) == INV          # new words need somewhere to go
    assert P(sc, 4, _lib.MgxResetSelect(None, p + 4), pool, *okp) == INV
    assert P(sc, 4, sel, pool, p + 1, p, p, p, p) == INV                                  # 16-bit cells: 2-byte aligned
    bad = spec.to_c()
    bad.cell_bytes = 5
    assert P(bad, 4, sel, pool, *okp) == INV
