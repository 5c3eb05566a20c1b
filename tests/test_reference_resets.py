"""Episode generation against the REFERENCE's own resets (tests/golden/resets_*.npz, written by oracle/gen_golden.py: record_resets
-- single unseeded reset() calls of ini/multigrid from given states of its two generators, one generator configuration per file).

The other layout tests pin the generators through a chain  HIP == oracle/mgx_layout_oracle.c == layouts.py == reference  whose last link
rests on eight resets of one size per env class.  Here every link is compared with the reference directly, at every size
`check_layout_gen` accepts, with pending 32-bit halves on either generator, and from CONSTRUCTED states at which numpy's bounded draw
really re-samples (Lemire's rejection: once in ~10^9 draws otherwise).  The coverage test counts, in the reference's own
instrumentation, the events the corpus exists for."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib, layouts, rng as rnglib
from oracle import binding as ob
from tests import util

FIX = dict(zip(util.RESETS_IDS, util.RESETS_GOLDEN))
CLASSES = ("empty_random", "empty_fixed", "blockedunlockpickup", "redbluedoors", "lockedhallway", "playground")


def load(name):
    z = np.load(FIX[name])
    d = json.loads(str(z["spec_json"]))
    return z, d, EnvSpec.from_dict(d), d["gen"]


def rooms_of(spec, gen):
    rs = gen["room_size"]
    return (spec.height - 1) // (rs - 1), (spec.width - 1) // (rs - 1)


def blank_of(spec, gen):
    kind = gen["kind"]
    if kind == "blockedunlockpickup":
        return layouts.roomgrid_blank(gen["room_size"], 1, 2)
    if kind == "redbluedoors":
        return layouts.redbluedoors_blank(spec.height)
    if kind == "lockedhallway":
        return layouts.lockedhallway_blank(2 * rooms_of(spec, gen)[0], gen["room_size"])
    if kind == "playground":
        return layouts.roomgrid_blank(gen["room_size"], *rooms_of(spec, gen))
    return layouts.empty_blank(spec.width)


def layouts_py(spec, gen, lay, npr):
    """multigrid_amd/layouts.py on numpy generators -> (grid, agents, target or None)"""
    kind, A = gen["kind"], spec.num_agents
    if kind == "blockedunlockpickup":
        return layouts.blockedunlockpickup_layout(gen["room_size"], A, lay, npr)
    if kind == "redbluedoors":
        return layouts.redbluedoors_layout(spec.height, A, lay) + (None,)
    if kind == "lockedhallway":
        return layouts.lockedhallway_layout(2 * rooms_of(spec, gen)[0], gen["room_size"], gen["max_hallway_keys"], gen["max_keys_per_room"],
                                            A, lay, npr) + (None,)
    if kind == "playground":
        return layouts.playground_layout(gen["room_size"], *rooms_of(spec, gen), A, lay, npr) + (None,)
    if kind == "empty_random":
        return layouts.empty_layout(spec.width, A, agent_start_pos=None, agent_start_dir=None, layout_rng=lay) + (None,)
    return layouts.empty_layout(spec.width, A, tuple(gen["start"][:2]), gen["start"][2]) + (None,)


def layout_oracle(spec, gen, lw, nw):
    """oracle/mgx_layout_oracle.c on generator words (advanced in place) -> (grid, agents, aux or None)"""
    kind, A, blank = gen["kind"], spec.num_agents, blank_of(spec, gen)
    if kind == "blockedunlockpickup":
        return ob.bup_layout(gen["room_size"], A, lw, nw, blank)
    if kind == "redbluedoors":
        return ob.rbd_layout(spec.height, A, lw, blank)
    if kind == "lockedhallway":
        return ob.lh_layout(2 * rooms_of(spec, gen)[0], gen["room_size"], gen["max_hallway_keys"], gen["max_keys_per_room"], A, lw, blank)
    if kind == "playground":
        return ob.playground_layout(gen["room_size"], *rooms_of(spec, gen), A, lw, nw, blank) + (None,)
    if kind == "empty_random":
        return ob.empty_random_layout(A, lw, blank) + (None,)
    g, a, _ = layouts_py(spec, gen, None, None)                       # (a fixed start draws nothing: there is no oracle entry for it)
    return g, a, None


def recorded_aux(z, gen, n):
    """The env's hook state (include/mgx.h aux) that belongs to recorded event n: from the reference's grid and target box."""
    kind = gen["kind"]
    if kind not in ("blockedunlockpickup", "redbluedoors", "lockedhallway"):
        return np.zeros(16, np.uint8)
    return layouts.make_aux(kind, z["grid0"][n], target=z["target"][n] if "target" in z.files else None)


@pytest.mark.parametrize("name", util.RESETS_IDS)
def test_layouts_py_reproduces_every_recorded_reset(name):
    z, d, spec, gen = load(name)
    for n in range(len(z["lay_before"])):
        lay, npr = rnglib.generator_from_gen_words(z["lay_before"][n]), rnglib.generator_from_gen_words(z["npr_before"][n])
        g, a, t = layouts_py(spec, gen, lay, npr)
        np.testing.assert_array_equal(g, z["grid0"][n], err_msg=f"{name} event {n}: grid")
        np.testing.assert_array_equal(a, z["agents0"][n], err_msg=f"{name} event {n}: agents")
        if t is not None:
            np.testing.assert_array_equal(t[:3], z["target"][n], err_msg=f"{name} event {n}: target")
        np.testing.assert_array_equal(rnglib.gen_words_from_generator(lay), z["lay_after"][n], err_msg=f"{name} event {n}: placement generator")
        np.testing.assert_array_equal(rnglib.gen_words_from_generator(npr), z["npr_after"][n], err_msg=f"{name} event {n}: np_random")


@pytest.mark.parametrize("name", util.RESETS_IDS)
def test_layout_oracle_reproduces_every_recorded_reset(name):
    z, d, spec, gen = load(name)
    for n in range(len(z["lay_before"])):
        lw, nw = z["lay_before"][n].copy(), z["npr_before"][n].copy()
        g, a, aux = layout_oracle(spec, gen, lw, nw)
        np.testing.assert_array_equal(g, z["grid0"][n], err_msg=f"{name} event {n}: grid")
        np.testing.assert_array_equal(a, z["agents0"][n], err_msg=f"{name} event {n}: agents")
        if aux is not None:
            np.testing.assert_array_equal(aux, recorded_aux(z, gen, n), err_msg=f"{name} event {n}: aux")
        np.testing.assert_array_equal(lw, z["lay_after"][n], err_msg=f"{name} event {n}: placement generator")
        np.testing.assert_array_equal(nw, z["npr_after"][n], err_msg=f"{name} event {n}: np_random")


@pytest.mark.parametrize("name", util.RESETS_IDS)
def test_reset_done_on_the_oracle_backend_reproduces_every_recorded_reset(name):
    """The host path of BatchedMultiGridEnv.reset_done() over device-side generation, on the CPU: generator states injected into
    `gen_state` / `rng`, every env finished -> the recorded start states, then gen_obs() -> the recorded first observation."""
    z, d, spec, gen = load(name)
    env = make_env(z, spec, gen, np.arange(len(z["lay_before"])), "cpu", backend=util.OracleBackend(spec))
    assert int(env.reset_done().sum()) == env.batch
    check_state(env, z, gen, np.arange(env.batch), name)
    env.gen_obs()
    np.testing.assert_array_equal(env.obs.numpy(), z["obs0"])


def make_env(z, spec, gen, idx, dev, staged=False, **kw):
    """A batch whose env b is recorded event idx[b] just before its reset: finished (step_count = max_steps), the two generators in
    the recorded states."""
    N = len(idx)
    env = BatchedMultiGridEnv(spec, N, dev, **kw)
    g0, a0, _ = layouts_py(spec, dict(gen, kind="empty_fixed") if gen["kind"] in ("empty_random", "empty_fixed") else gen,
                           np.random.default_rng(1), np.random.default_rng(2))
    aux0 = None
    if spec.env_kind != "empty":
        aux0 = layouts.make_aux(spec.env_kind, g0, target=np.array([7, 0, 0, 0], np.uint8))
    env.load_state(g0, a0, aux=aux0)
    env.set_layout_generator(gen["kind"], layout_seed=1, room_size=gen["room_size"], start=tuple(gen["start"]),
                             max_hallway_keys=gen["max_hallway_keys"], max_keys_per_room=gen["max_keys_per_room"], staged=staged)
    inject(env, z, idx)
    env.step_count.fill_(spec.max_steps)
    return env


def inject(env, z, idx):
    gs = np.zeros((len(idx), 6), np.uint64)
    gs[:, :5] = z["lay_before"][idx]
    gs[:, 5] = z["npr_before"][idx, 4]
    env._gen["gen_state"].copy_(torch.from_numpy(gs.view(np.int64)))
    env.rng.copy_(torch.from_numpy(np.ascontiguousarray(z["npr_before"][idx, :4]).view(np.int64)))


def check_state(env, z, gen, idx, ctx, episode=1):
    """the env's state tensors == the recorded bytes of events idx"""
    def same(got, want, what):
        got = got.cpu()
        want = torch.from_numpy(np.ascontiguousarray(want))
        if not torch.equal(got, want.view(got.dtype) if want.dtype != got.dtype else want):
            bad = (got.reshape(len(idx), -1) != want.view(got.dtype).reshape(len(idx), -1)).any(-1).nonzero().flatten()[:4].tolist()
            raise AssertionError(f"{ctx}: {what} differs from the reference's, envs {bad} (events {[int(idx[b]) for b in bad]})")
    same(env.grid, z["grid0"][idx], "grid")
    same(env.agents, z["agents0"][idx], "agents")
    if env.spec.env_kind != "empty":
        same(env.aux, np.stack([recorded_aux(z, gen, n) for n in idx]), "aux")
    same(env.rng, z["npr_after"][idx, :4].view(np.int64), "rng (np_random)")
    gs = env._gen["gen_state"].cpu().numpy().view(np.uint64)
    same(torch.from_numpy(gs[:, :5].copy().view(np.int64)), z["lay_after"][idx].view(np.int64), "gen_state[:, :5] (placement generator)")
    same(torch.from_numpy(gs[:, 5].copy().view(np.int64)), z["npr_after"][idx, 4].copy().view(np.int64), "gen_state[:, 5] (np_random's 32-bit buffer)")
    same(env.step_count, np.zeros(len(idx), np.int32), "step_count")
    same(env.episode, np.full(len(idx), episode, np.int32), "episode")
    same(env.was_reset, np.ones(len(idx), np.uint8), "was_reset")


def accepted(spec, gen) -> bool:
    """Does the product take this generator configuration (mgx_layout_gen.h check_layout_gen, asked through mgx_reset_generate without a
    launch)?  The check answers MGX_ERR_UNSUPPORTED for a layout that may not exist.  Behind it the call stops with
    MGX_ERR_INVALID_ARGUMENT before any launch: for a hook env because `aux` is missing; for the hook-free kinds (Empty, Playground),
    which would launch, the same question is asked with the spec's env_kind swapped for a hook kind -- the feasibility conditions do
    not read it, the shape conditions behind them refuse it.  (That the hook-free SHAPES are accepted is what the GPU tests show by
    running every one of them.)"""
    import dataclasses
    rs = gen["room_size"]
    hook_free = spec.env_kind == "empty"
    sc = (dataclasses.replace(spec, env_kind="redbluedoors", joint_reward=True) if hook_free else spec).to_c()
    g = _lib.MgxLayoutGen(_lib.GEN_KINDS[gen["kind"]], rs, *gen["start"], gen["max_hallway_keys"], gen["max_keys_per_room"], 4096, 4096)
    rc = _lib.lib().mgx_reset_generate(C.byref(sc), 8, C.byref(g), 4096, 4096, 4096, 4096, None, 4096, None, None)
    assert rc in (_lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED), rc
    return rc == _lib.ERR_INVALID_ARGUMENT


def test_every_recorded_configuration_is_one_the_product_accepts():
    assert len(util.RESETS_IDS) >= 30
    for name in util.RESETS_IDS:
        z, d, spec, gen = load(name)
        assert accepted(spec, gen), name
    # (the probe itself: a configuration the product refuses is told apart)
    spec = EnvSpec(7, 4, 3, 3, max_steps=9, joint_reward=True, env_kind="blockedunlockpickup")
    assert not accepted(spec, dict(kind="blockedunlockpickup", room_size=4, max_hallway_keys=1, max_keys_per_room=2, start=[1, 1, 0]))
    gen = lambda kind, rs=0: dict(kind=kind, room_size=rs, max_hallway_keys=1, max_keys_per_room=2, start=[1, 1, 0])
    assert not accepted(EnvSpec(4, 4, 4, 3, max_steps=9), gen("empty_random"))                       # 2x2 interior: goal + 4 agents
    assert not accepted(EnvSpec(11, 11, 4, 7, max_steps=9), gen("playground", 6))                    # 12 objects + 4 agents + 1 > 16 cells
    # a Playground whose START room cannot hold 12 objects away from the agents' start (size 6: 11 such cells) -- the reference raises
    # RecursionError when all 12 draw it, the device would never return: refused where that is certain or likely (fewer than 4 rooms)
    assert not accepted(EnvSpec(6, 6, 1, 5, max_steps=9), gen("playground", 6))
    assert not accepted(EnvSpec(11, 6, 2, 5, max_steps=9), gen("playground", 6))
    assert accepted(EnvSpec(7, 7, 1, 5, max_steps=9), gen("playground", 7)) and accepted(EnvSpec(11, 11, 2, 5, max_steps=9), gen("playground", 6))


def test_the_corpus_holds_the_events_it_exists_for():
    """Counts over the REFERENCE's own instrumentation (oracle/gen_golden.py: _ResetProbe): conditions on the inputs, not tolerances.
    Each minimum is a round figure below what the recorder's deterministic search finds; a corpus that loses one of these kinds of
    event no longer tests what it was made for."""
    n = dict.fromkeys(("events", "pending", "tries>8", "tries>16", "before", "before in a later round", "later", "low", "high",
                       "outside", "np_random", "np_random high", "np_random low", "shuffle rejected", "shuffle pending",
                       "keys min", "keys max", "rooms shared"), 0)
    per_class = {k: dict(before=0, later=0, second=0, full=0) for k in CLASSES}
    candidates = {k: set() for k in CLASSES}
    for name in util.RESETS_IDS:
        z, d, spec, gen = load(name)
        kind, A, rs = gen["kind"], spec.num_agents, gen["room_size"]
        c, r, s = z["calls"], z["resamples"], z["shuffles"]
        lay_r = r[r[:, 1] == 0]
        n["events"] += len(z["lay_before"])
        n["pending"] += int((((z["lay_before"][:, 4] | z["npr_before"][:, 4]) >> np.uint64(32)) != 0).sum())
        n["tries>8"] += int((c[:, 1] > 8).sum()); n["tries>16"] += int((c[:, 1] > 16).sum())
        grouped = (c[:, 2] >= 2) & (c[:, 3] >= 2)               # (calls the groups of eight take: both spans draw)
        n["before"] += int((grouped & (c[:, 4] > 0)).sum())
        n["before in a later round"] += int((grouped & (c[:, 4] > 0) & (c[:, 1] > 8)).sum())
        n["later"] += int(c[:, 5].sum())
        n["low"] += int((lay_r[:, 4] == 0).sum()); n["high"] += int((lay_r[:, 4] == 1).sum())
        n["outside"] += int((lay_r[:, 5] == 0).sum())
        npr_r = r[r[:, 1] == 1]
        assert len(npr_r) == 0 or kind == "blockedunlockpickup"
        n["np_random"] += len(npr_r); n["np_random high"] += int((npr_r[:, 4] == 1).sum()); n["np_random low"] += int((npr_r[:, 4] == 0).sum())
        n["shuffle rejected"] += int((s[:, 2] > 0).sum()); n["shuffle pending"] += int((s[:, 3] > 0).sum())
        per_class[kind]["before"] += int((grouped & (c[:, 4] > 0)).sum()); per_class[kind]["later"] += int(c[:, 5].sum())
        per_class[kind]["second"] += int((c[:, 1] > 8).sum())
        if kind == "lockedhallway":
            kd = z["key_draws"]
            assert len(kd) and (kd[:, 2] >= 1).all() and (kd[:, 2] <= kd[:, 1]).all()
            n["keys min"] += int((kd[:, 2] == 1).sum()); n["keys max"] += int(((kd[:, 2] == kd[:, 1]) & (kd[:, 1] > 1)).sum())
        if kind == "playground":
            n["rooms shared"] += sum(len(set(row)) < len(row) for row in z["object_rooms"].tolist())
        # mgx_layout_gen.h stage_candidates: one candidate per value of the generator's np_random draw (0: the snapshot protocol)
        candidates[kind].add((rs - 2 if rs - 2 <= 4 else 0) if kind == "blockedunlockpickup" else 0 if kind == "playground" else 1)
        W, H = spec.width, spec.height
        room = (rs - 2) ** 2
        per_class[kind]["full"] += {"empty_random": (W - 2) * (H - 2) - 1 == A, "blockedunlockpickup": room == A + 2,
                                    "redbluedoors": (W // 2 - 2) * (H - 2) == A,
                                    "lockedhallway": (rs - 2) * (H - 2) == A + gen["max_hallway_keys"]}.get(kind, False)
    print(n, per_class, candidates)
    assert 2 * n["pending"] >= n["events"] >= 400                # half of the events start on a pending 32-bit half
    assert n["tries>8"] >= 150 and n["tries>16"] >= 50          # a second / a third round of a group of eight
    assert n["before"] >= 40 and n["before in a later round"] >= 10     # a real re-sample at or before the first fit: serial fallback
    assert n["later"] >= 25                                      # a later try of the fitting group claims one: must be ignored
    assert n["low"] >= 25 and n["high"] >= 25                   # the rejected draw was a word's low half / a pending high half
    assert n["outside"] >= 10                                    # colour, direction, room and key-count draws that re-sampled
    assert n["np_random"] >= 6 and n["np_random high"] >= 2 and n["np_random low"] >= 2      # BlockedUnlockPickup's door row
    assert n["shuffle rejected"] >= 80 and n["shuffle pending"] >= 80
    assert n["keys min"] >= 100 and n["keys max"] >= 60 and n["rooms shared"] >= 50
    for kind in CLASSES:
        if kind != "empty_fixed":                                # (a fixed start draws nothing)
            assert per_class[kind]["before"] >= 5 and per_class[kind]["later"] >= 2 and per_class[kind]["second"] >= 15, (kind, per_class[kind])
    for kind in ("empty_random", "blockedunlockpickup", "redbluedoors", "lockedhallway"):
        assert per_class[kind]["full"] >= 1, kind
    assert candidates["blockedunlockpickup"] == {0, 2, 3, 4} and candidates["playground"] == {0}
    assert all(candidates[k] == {1} for k in ("empty_random", "empty_fixed", "redbluedoors", "lockedhallway"))


# ---- chained episodes (tests/golden/resets_chain_*.npz) ---------------------------------------------------------------------------
CHAINS = dict(zip(util.RESETS_CHAIN_IDS, util.RESETS_CHAIN_GOLDEN))


def load_chain(name):
    z = np.load(CHAINS[name])
    d = json.loads(str(z["spec_json"]))
    return z, d, EnvSpec.from_dict(d), d["gen"]


def chain_aux(z, gen, r):
    if gen["kind"] != "blockedunlockpickup":
        return np.zeros(16, np.uint8)
    return layouts.make_aux("blockedunlockpickup", z["grid0"][r], target=z["target"][r])


@pytest.mark.parametrize("name", util.RESETS_CHAIN_IDS)
def test_chain_replays_through_the_dict_api_on_the_oracle_backend(name):
    """mg.make(..., device="cpu", _backend=OracleBackend) with the two generator states injected: every step's outputs, the state
    each step leaves, and every unseeded reset -- after truncations and after early ends alike -- equal the reference's."""
    import multigrid_amd as mg
    z, d, spec, gen = load_chain(name)
    A = spec.num_agents
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in d["make"].items()}
    env = mg.make(d["env_id"], device="cpu", _backend=lambda sp: util.OracleBackend(sp), **kw)
    env.reset(seed=0)
    env._layout_rng = rnglib.generator_from_gen_words(z["lay0"])
    env._np_random = rnglib.generator_from_gen_words(z["npr0"])
    env._rng_on_device = False

    def check_reset(r, obs):
        ctx = f"{name} reset {r}"
        np.testing.assert_array_equal(env._benv.grid[0].numpy(), z["grid0"][r], err_msg=ctx)
        np.testing.assert_array_equal(env._benv.agents[0].numpy(), z["agents0"][r], err_msg=ctx)
        for i in range(A):
            np.testing.assert_array_equal(obs[i]["image"], z["obs0"][r][i], err_msg=ctx)
        if gen["kind"] == "blockedunlockpickup":
            np.testing.assert_array_equal(env._benv.aux[0].numpy()[:3], z["target"][r], err_msg=ctx)
        np.testing.assert_array_equal(rnglib.gen_words_from_generator(env._layout_rng), z["lay_after"][r], err_msg=ctx)
        np.testing.assert_array_equal(rnglib.gen_words_from_generator(env._np_random), z["npr_after"][r], err_msg=ctx)
        np.testing.assert_array_equal(env._benv.rng[0].numpy().view(np.uint64), z["npr_after"][r, :4], err_msg=ctx)

    obs, _ = env.reset()
    check_reset(0, obs)
    edits = {int(t): row for t, row in zip(z["edit_step"], z["edit_row"])}
    for t in range(len(z["actions"])):
        ctx = f"{name} step {t}"
        if t in edits:
            env._benv.agents[0, 0] = torch.from_numpy(edits[t].copy())
        obs, rew, term, trunc, _ = env.step({i: int(a) for i, a in enumerate(z["actions"][t])})
        for i in range(A):
            np.testing.assert_array_equal(obs[i]["image"], z["obs"][t][i], err_msg=ctx)
            assert obs[i]["direction"] == z["dir"][t][i] and rew[i] == z["reward"][t][i], ctx
            assert term[i] == bool(z["terminated"][t][i]) and trunc[i] == bool(z["truncated"][t]), ctx
        np.testing.assert_array_equal(env._benv.grid[0].numpy(), z["grid"][t], err_msg=ctx)
        np.testing.assert_array_equal(env._benv.agents[0].numpy(), z["agents"][t], err_msg=ctx)
        np.testing.assert_array_equal(env._benv.rng[0].numpy().view(np.uint64), z["npr"][t, :4], err_msg=ctx)
        assert bool(env.is_done()) == bool(z["done"][t]), ctx
        if z["done"][t]:
            obs, _ = env.reset()
            check_reset(int(z["reset_of"][t]), obs)


def test_every_chain_holds_early_ends_and_truncations():
    assert len(util.RESETS_CHAIN_IDS) >= 5
    kinds = set()
    for name in util.RESETS_CHAIN_IDS:
        z, d, spec, gen = load_chain(name)
        assert accepted(spec, gen), name
        done, trunc = z["done"].astype(bool), z["truncated"].astype(bool)
        assert (trunc <= done).all() and int(done.sum()) + 1 == len(z["grid0"]), name
        early = done & ~trunc
        assert int(early.sum()) >= 4 and int(trunc.sum()) >= 4, (name, int(early.sum()), int(trunc.sum()))
        assert set(z["edit_step"].tolist()) == set(np.nonzero(early)[0].tolist()), name      # every early end is an edited step
        # the early ends fall on different steps of their episodes, and rewards are paid at them
        starts = np.concatenate([[0], np.nonzero(done)[0] + 1])
        at = {int(t - starts[starts <= t].max()) for t in np.nonzero(early)[0]}
        assert len(at) >= 3, (name, at)
        assert (z["reward"][early] > 0).any(axis=1).all(), name
        assert (z["lay0"][4] >> np.uint64(32)) == 1 and (z["npr0"][4] >> np.uint64(32)) == 1, name
        kinds.add((gen["kind"], spec.height))
    assert {k for k, _ in kinds} == {"blockedunlockpickup", "empty_random"}
    assert {h for k, h in kinds if k == "blockedunlockpickup"} >= {5, 6, 8}              # 3 / 4 candidates and the `between` fallback
