"""Random call sequences through BatchedMultiGridEnv on the HIP backend (the driver: tests/env_sequences.py; the same lists on two
oracle-backed envs: tests/test_env_sequences.py).

  * HIP against the oracle: one env on `HipBackend`, its twin on the CPU model of every launcher (`SeqOracle`); the lists of the CPU
    file with the GPU-only kinds switched on -- a captured graph replayed twice, a graph kept and replayed again later, a persistent
    session, step(sub_shards=2) + join(); every member compared byte for byte after every call, both marker rules on the HIP env;
  * the time machine on the device, where it also covers the staged generator's slots;
  * the size that READS the layout marker: 32 784 envs (more than 2048 wavefronts) on a one-layout pool, against a second HIP env whose
    steps are bound untracked (`_tracks` replaced on the instance): every third call a step(auto_reset=True) that would trust a
    stale marker, cell edits that land in marked envs and change what they observe;
  * the pinned cases of the CPU file against the oracle;
  * the forms `plain_jit` and `pool1_jit`: one list each on a HIP env whose step kernel is compiled at run time and registered;
  * the query layer on (make_ops(queries=True)): behind every call zero to two read-only calls -- row queries of the env and of kept
    snapshots, obs_key, a key table, a selection, and all of them captured into one graph that is kept and replayed later --, their
    answers among the members compared.  A step(sub_shards=2) directly in front of a query is not joined by the driver: the query
    is the chains' first consumer, and nothing here reads the HIP env in between.  What the twin cannot show, because it runs the
    same host logic, is asserted on the HIP env's host state: a query leaves `_mark["armed"]` as it was and `_chains_pending` off,
    and a snapshot's rows answer as the launcher does over the snapshot's own tensors (test_env_sequences.asked_directly).
  * the hook forms (es.HOOK_FORMS): RedBlueDoors, LockedHallway, Playground's generator and the declared rules through the same lists
    -- `aux` is among the members compared after every call, so an adoption, a restore or a pool restart that loses hook state
    shows here; the stepping calls of the RedBlueDoors and LockedHallway forms come with a visiting order through step(), step(
    sub_shards=2), split() children and capture_steps(sub_shards=1 or 2).  Asserted on the HIP env: a restore / reset(mask) / seed
    met a live slot (the three generator forms), auto-reset steps ran the tracked entry (the pool forms), and a step with a
    visiting order met an armed marker (rbd_pool, lh_pool).  The mutants tried for these forms: tests/test_env_sequences.py.

Recorded host-logic mutants of multigrid_amd/batched.py (none committed, none touches a kernel, all in bounds), each tried on both
sequence files, one run each:

  1. `_row_set` hands out `self.cells` instead of `self._cells`.
     CPU file: dies.  The read-only fingerprint fails ("a query wrote ['_marker', 'armed']") in the 8 sequence cases and the 2
     census cases of pool1 and pool1_jit, at the first query of an armed env; the oracle envs of the other forms are never armed.
     This file, as it stood then: test_the_size_that_reads_the_marker[big_objects1-2] alone ("no cell edit landed in a marked env");
     45 others passed -- the answers are right either way.  The assertion on `_mark["armed"]` around every query was added for it
     (not run against the mutant).
  2. `_copy_entry` without its `join()`.
     CPU file: cannot catch it (the oracle has no chains): 72 passed.
     This file, as it stood then: SURVIVED, 46 passed -- no query behind unjoined chains read half a step in that run; a race, and
     it was not run again to make it show.  The assertion on `_chains_pending` after every query was added for it and kills it
     without a race: of 10 cases run (pool1, gen_between, the marker size) the 7 whose lists hold a first consumer failed, "the
     query did not join the sub-shard chains".
  3. `EnvSnapshot._row_set` launches over the tensors of the env as it is now instead of the snapshot's own.
     CPU file: dies in all 40 sequence cases and the 10 census cases ("not the answer of the rows it names": asked_directly).
     This file, as it stood then: SURVIVED, 46 passed -- the twin runs the same host logic and gives the same wrong answer.  The
     asked_directly check of q_snap on the twin was added here too (the check the CPU file runs; not run against the mutant here)."""
import functools

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, jit, layouts, rng as rnglib
from tests import env_sequences as es
from tests.test_env_sequences import asked_directly, time_machine
from tests.test_grid_layout_marker import THROUGHPUT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEQUENCES = [(130, 1), (130, 2), (7, 4)]
N_OPS = 120


def live_slots(env, op) -> int:
    """how many of the envs this call writes hold a staging slot whose tag is live (not the empty value), read just before it"""
    st = (getattr(env, "_gen", None) or {}).get("stage")
    if st is None or op["kind"] not in ("restore", "reset", "seed"):
        return 0
    tag = st["tag"].cpu()
    live = (tag != -1).any(dim=1) if st.get("candidates") else tag[:, 0] != -1
    if op["kind"] == "restore" and op["env_ids"] is not None:
        return int(live[torch.from_numpy(op["env_ids"])].sum())
    if op["kind"] == "reset" and op["mask"] is not None:
        return int(live[torch.from_numpy(op["mask"].astype(bool))].sum())
    return int(live.sum())


@functools.lru_cache(maxsize=None)
def sequence(form, B, seed):
    ops = es.make_ops(form, B, N_OPS, seed, gpu=True, queries=True)
    jit_form = form in es.JIT_FORMS                           # (the HIP env steps on a kernel compiled for its shape at run time)
    hip, twin = es.make_env(form, B, DEV, specialise=jit_form), es.make_env(form, B, specialise=jit_form)
    ch, ct = es.new_ctx(), es.new_ctx()
    seen = {"live_slots": 0, "tracked_entry": False, "shape_kernel": (hip.shape_kernel, twin.shape_kernel),
            "fixed_shape": hip.backend.launch_info(B)["fixed_shape"]}
    for i, op in enumerate(ops):
        where = es.where_text(form, B, seed, i, ops)
        nxt = es.following(ops, i)
        seen["live_slots"] += live_slots(hip, op)
        armed = hip._mark["armed"]
        oh, ot = es.apply(hip, op, ch, nxt), es.apply(twin, op, ct, nxt)
        if op["kind"] in es.QUERY_KINDS:
            # the host's side of a query, which the twin shares and so cannot show: the marker's flag stays, a first consumer has
            # joined the chains, and a snapshot's rows answer as the launcher does over the snapshot's own tensors
            assert hip._mark["armed"] == armed, f"{where}: the query changed whether the layout marker is armed"
            assert not hip._chains_pending, f"{where}: the query did not join the sub-shard chains"
            if op["kind"] == "q_snap":
                (got,), want = [v for k, v in ot.items() if k.startswith("out.")], asked_directly(twin, op, ct)
                assert got.numpy().tobytes() == want.numpy().tobytes(), f"{where}: not the answer of the snapshot's own rows"
        es.invariants(twin, where)
        es.check_shadow(twin, where)
        if es.unjoined(op, nxt):
            # the chains are still running and the query behind them is their first consumer: nothing here may read the HIP env (it
            # would wait for nothing and read half a step); state and outputs of this step are compared after that query
            continue
        es.invariants(hip, where)
        es.compare(hip, twin, ch, ct, where, oh, ot)
        ent = hip._bound.get((True, False))
        seen["tracked_entry"] = seen["tracked_entry"] or bool(ent and ent[2])
    seen["order_while_armed"] = ch["seen"].get("stepped_with_hook_order_while_armed", 0)      # (counted on the HIP env's own flag)
    return ops, twin.backend, seen


@pytest.mark.parametrize("B,seed", SEQUENCES)
@pytest.mark.parametrize("form", es.FORMS)
def test_hip_equals_the_oracle_after_every_call(form, B, seed):
    ops, be, seen = sequence(form, B, seed)
    assert len(es.without_queries(ops)) == N_OPS and len(ops) > N_OPS


@pytest.mark.skipif(not jit.hiprtc_available(), reason="no libhiprtc")
@pytest.mark.parametrize("form", es.JIT_FORMS)
def test_a_registered_shape_equals_the_oracle_after_every_call(form):
    """`plain` and `pool1` on shapes whose kernel is compiled at run time and registered (tests/test_jit_forms_gpu.py has the other
    forms such a kernel serves): every step of the list without a one-hot output, its auto-reset steps included, runs it."""
    ops, be, seen = sequence(form, 130, 1)
    assert len(es.without_queries(ops)) == N_OPS and len(ops) > N_OPS
    kinds = [o["kind"] for o in ops]
    assert all(kinds.count(k) >= 1 for k in es.legal_query_kinds(form, 130, True) if k != "q_graph_again"), \
        "a query kind never ran on the run-time-compiled shape"
    assert seen["shape_kernel"][0] in ("compiled", "registered") and seen["shape_kernel"][1] is None
    assert seen["fixed_shape"] == 100, "the launches of this batch do not run the registered kernel"      # MGX_SHAPE_RUNTIME_COMPILED
    assert sum(o["kind"] == "step" for o in ops) >= 3
    assert any(o["kind"] == "step" and o["auto_reset"] for o in ops) == (form == "pool1_jit")


@pytest.mark.parametrize("form", es.FORMS)
def test_census(form):
    runs = [sequence(form, B, seed) for B, seed in SEQUENCES]
    c = es.census_of([r[0] for r in runs], [r[1] for r in runs])
    es.assert_census(c, form, 130, gpu=True, queries=True)
    if form in ("gen_candidates", "gen_between", "bup_candidates", "rbd_candidates", "lh_candidates", "playground_between"):
        assert sum(r[2]["live_slots"] for r in runs) > 0, "no restore / reset(mask) / seed met a live staging slot"
    if form in ("pool1", "pool4_objects") + es.HOOK_POOL_FORMS:
        assert any(r[2]["tracked_entry"] for r in runs), "step(auto_reset=True) never ran through the tracked hot-path entry"
    if form in es.ORDERED_POOL_FORMS:       # (here the marker is armed by the tracked steps themselves, at every pool size)
        assert sum(r[2]["order_while_armed"] for r in runs) > 0, "no step with a visiting order met an armed layout marker"


@pytest.mark.parametrize("form", es.FORMS)
def test_time_machine(form):
    kinds = {o["kind"] for o in time_machine(form, 130, 5, device=DEV, gpu=True)}
    assert kinds <= set(es.PURE_KINDS) and "step" in kinds and "restore" in kinds


@pytest.mark.parametrize("name", list(es.PINNED))
def test_pinned(name):
    case = es.PINNED[name]()
    form, B, ops = case["form"], case["B"], case["ops"]
    hip, twin = es.make_env(form, B, DEV), es.make_env(form, B)
    ch, ct = es.new_ctx(), es.new_ctx()
    for i, op in enumerate(ops):
        where = f"pinned case {name}: call {i}: {es.describe(op)}"
        oh, ot = es.apply(hip, op, ch), es.apply(twin, op, ct)
        es.invariants(hip, where)
        es.compare(hip, twin, ch, ct, where, oh, ot)
        if i in case.get("checks", {}):
            case["checks"][i](hip, where)


# ---- the size that reads the marker -------------------------------------------------------------------------------------------------

BIG_KINDS = ("step", "step_one_hot", "rollout", "reset_done", "reset", "snapshot", "snapshot_out", "restore", "fork", "edit",
             "pool_refill", "track", "reset_totals", "seed", "gen_obs", "one_hot_obs", "split", "capture_replay", "graph_again",
             "step_chains")
#: the query layer at this size, with small weights: the row queries (of the env and of kept snapshots, at most es.MAX_QUERY_ROWS ids and 40 rows a call) and
#: the selection (one pass over the first 4096 envs); the tracked env and its untracked twin must answer alike
BIG_QUERY_KINDS = ("q_state_key", "q_action_mask", "q_distance", "q_snap", "q_select")
BIG_KINDS += BIG_QUERY_KINDS
BIG_WEIGHTS = {"edit": 6, "rollout": 4, "restore": 4, "snapshot": 3, "capture_replay": 3, "graph_again": 2, "track": 1, "step": 3,
               "q_state_key": 1, "q_action_mask": 1, "q_distance": 1, "q_snap": 1, "q_select": 1}


def big_env(form, tracked):
    spec, B = es.SPECS[form], THROUGHPUT
    if form == "big_empty1":
        g, a = layouts.empty_layout(16, 4)
        g, a = g[None].copy(), a[None].copy()
    else:
        g, a, _ = es.object_pool(spec, 1, 11)
    env = BatchedMultiGridEnv(spec, B, DEV)
    if not tracked:
        env._tracks = lambda: False                          # (on the instance: its steps bind the untracked entry, mgx_step_ex)
        split = env.split

        def untracked_split(parts):                          # (... and so do the steps of its sub-shards, capture_steps' included)
            children = split(parts)
            for c in children:
                c._tracks = env._tracks
            return children
        env.split = untracked_split
    k = np.zeros(B, np.int64)
    env.load_state(g[k], a[k], rng=rnglib.synthetic_words(B, 3, 0), step_count=(np.arange(B) % spec.max_steps).astype(np.int32))
    env.set_layout_pool(g, a)
    return env


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("form", es.BIG_FORMS)
def test_the_size_that_reads_the_marker(form, seed):
    B = THROUGHPUT
    ops = es.make_ops(form, B, 40, seed, gpu=True, kinds=BIG_KINDS, weights=BIG_WEIGHTS, every_third=True, queries=True)
    assert len(es.without_queries(ops)) == 40 and {o["kind"] for o in ops} & set(BIG_QUERY_KINDS)
    env, twin = big_env(form, True), big_env(form, False)
    assert env.backend.launch_info(B)["envs_per_wavefront"] * 2048 < B, "not the family of launches that reads the marker"
    assert int((env._marker == 0).sum()) == B and int((twin._marker >= 0).sum()) == 0
    ce, ct = es.new_ctx(), es.new_ctx()
    edits_in_marked_envs = tracked_entry = 0
    for i, op in enumerate(ops):
        where = es.where_text(form, B, seed, i, ops)
        if op["kind"] == "edit":                              # the negative control: the edit lands in marked envs, and shows
            ids = torch.from_numpy(op["env_ids"]).to(DEV)
            marked = env._marker[ids] >= 0
            before = env.gen_obs()[0][ids].clone()
            twin.gen_obs()
        nxt = es.following(ops, i)
        armed = env._mark["armed"]
        oe, ot = es.apply(env, op, ce, nxt), es.apply(twin, op, ct, nxt)
        if op["kind"] in es.QUERY_KINDS:                      # (a query keeps the marker's promises, and joins)
            assert env._mark["armed"] == armed and not env._chains_pending, where
        if op["kind"] == "edit":
            after = env.gen_obs()[0][ids]
            twin.gen_obs()
            edits_in_marked_envs += int((marked & (before != after).flatten(1).any(dim=1)).sum())
        if es.unjoined(op, nxt):                              # (the chains are left to the query behind them: sequence() above)
            continue
        es.invariants(env, where)
        es.compare(env, twin, ce, ct, where, oe, ot, to_host=False)
        ent, tent = env._bound.get((True, False)), twin._bound.get((True, False))
        tracked_entry += int(bool(ent and ent[2]))
        assert not (tent and tent[2]), "the twin's steps keep the marker: it is no reference"
    assert tracked_entry > 0, "step(auto_reset=True) never ran through mgx_step_tracked"
    assert edits_in_marked_envs > 0, "no cell edit landed in a marked env and changed what it observes"
    assert sum(o["kind"] == "step" and o["auto_reset"] for o in ops) >= 13
