"""Record SEEDED resets of the real reference: tests/golden/seeded/seeded_resets.npz, the truth BatchedMultiGridEnv.reset(seed=...) is held to.

    python tools/record_seeded_resets.py          (CPU only; needs the reference checkout, $MGX_REFERENCE)

`env.reset(seed=s)` of the reference (multigrid/base.py:250-301) replaces env.np_random with Generator(PCG64(SeedSequence(s))) and
leaves the construction-time placement generator alone; the reset corpus of oracle/gen_golden.py (resets_*.npz) holds unseeded resets
only.  Here, for each of the six generator kinds at its smallest recorded size, four reset(seed=s) calls are made from given states
of BOTH generators -- event i starts with a pending 32-bit half on the placement generator when i & 1 and on np_random when i & 2
(the latter must not survive the re-seed) -- and stored with the conventions of resets_*.npz, every key prefixed "<tag>.":

    seed i64[N]   lay_before, npr_before u64[N,5]   grid0 u8[N,H,W,3]   agents0 u8[N,A,8]   obs0 u8[N,A,v,v,3]
    target u8[N,3] (BlockedUnlockPickup)            lay_after, npr_after u64[N,5]           spec_json (EnvSpec fields + "gen")

The reference is imported the way oracle/gen_golden.py does -- through that module's own sys.path lines ($MGX_REFERENCE,
oracle/standins) --; nothing under oracle/ changes.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from oracle import gen_golden as gg  # noqa: E402  (puts the reference checkout and oracle/standins on sys.path, as it does for itself)
import multigrid.envs as ref_envs  # noqa: E402
from multigrid_amd import layouts  # noqa: E402

#: (a directory of its own: tests/util.py takes every tests/golden/*.npz it does not know by prefix for a step trajectory)
OUT = os.path.join(REPO, "tests", "golden", "seeded", "seeded_resets.npz")
TAGS = ("empty_fixed_5_a3", "empty_random_6_a3", "bup_rs5_a2", "rbd_5_a2", "lh_2rooms_rs5_k33_a2", "playground_1x1_rs7_a1")
SEEDS = (7, 0, 12345, (1 << 31) + 5)


def main():
    configs = {c[0]: c for c in gg.RESET_CONFIGS}
    rec = {}
    for n, tag in enumerate(TAGS):
        _, kind, cls_name, kw, _ = configs[tag]
        cls = getattr(ref_envs, cls_name)
        cls._default_seed = 0x5EED00 + n
        env = cls(**kw)
        env.reset(seed=n)
        A = env.num_agents
        events = []
        for i, seed in enumerate(SEEDS):
            lay_state, npr_state = gg._reset_pre_states(tag, i)
            lay = env._RandomMixin__np_random
            lay.bit_generator.state, env.np_random.bit_generator.state = lay_state, npr_state
            ev = dict(seed=np.int64(seed), lay_before=gg._gen_words5(lay), npr_before=gg._gen_words5(env.np_random))
            obs, _ = env.reset(seed=seed)
            assert env._RandomMixin__np_random is lay, "reset(seed) replaced the placement generator"
            fresh = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))
            assert gg._gen_words5(env.np_random)[2:4].tolist() == gg._gen_words5(fresh)[2:4].tolist(), "np_random is not SeedSequence(seed)'s"
            ev.update(grid0=layouts.grid_to_product(gg.grid_with_contents(env)), agents0=layouts.pack_agents(gg.agents_with_contents(env)),
                      obs0=np.stack([obs[a]["image"] for a in range(A)]).astype(np.uint8), lay_after=gg._gen_words5(lay),
                      npr_after=gg._gen_words5(env.np_random))
            if kind == "blockedunlockpickup":
                ev["target"] = np.array([int(v) for v in np.asarray(env.obj)], dtype=np.uint8)
            events.append(ev)
        for k in events[0]:
            a = np.stack([e[k] for e in events])
            rec[f"{tag}.{k}"] = a.astype(np.uint8) if k in ("grid0", "agents0", "obs0") else a
        gen = dict(kind=kind, room_size=int(kw.get("room_size", 0)), max_hallway_keys=int(kw.get("max_hallway_keys", 1)),
                   max_keys_per_room=int(kw.get("max_keys_per_room", 2)),
                   start=[int(v) for v in (*(kw.get("agent_start_pos", (1, 1)) or (1, 1)), kw.get("agent_start_dir", 0))])
        env_kind = kind if kind in ("blockedunlockpickup", "redbluedoors", "lockedhallway") else "empty"
        rec[f"{tag}.spec_json"] = np.array(json.dumps(dict(gg.spec_of_noreset(env, env_kind), gen=gen)))
        pend = rec[f"{tag}.npr_before"][:, 4] >> np.uint64(32)
        print(f"{tag:28s} events={len(events)} pending np_random halves before={int(pend.sum())} after={int((rec[f'{tag}.npr_after'][:, 4] >> np.uint64(32)).sum())}")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **rec)
    size = os.path.getsize(OUT)
    print(f"{OUT}: {size / 1024:.1f} KiB")
    assert size <= 64 << 10


if __name__ == "__main__":
    main()
