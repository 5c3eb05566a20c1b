"""Random call sequences through BatchedMultiGridEnv on the oracle backend (no GPU): the driver is tests/env_sequences.py.

Every feature of batched.py that keeps engine state beside the public state -- the layout marker and its host flags, the staged
generator's slots, reset(seed, mask), the episode accounting, snapshot / restore / fork -- has a suite of its own that walks a script
written for it.  Here the calls come in arbitrary order:

  * sequences: per form (the two of es.JIT_FORMS included: on the oracle they are `plain` and `pool1` on grids that are not square)
    three seeds of 120 calls at 130 envs and one at 7.  After every call the layout marker's two rules hold
    (env_sequences.invariants), EpisodeStats equals what the launches' own outputs make of it (SeqOracle.shadow: the accounting
    launch follows every stepping and restart form), and a second env given the same list holds the same bytes;
  * census: over a form's seeds every legal call kind ran at least three times, and the restarts, restores and switches that the
    cross-feature rules are about happened;
  * time machine: snapshot() of the whole batch, thirty to sixty calls, restore(), the same calls again: every recorded output and
    the final state are equal -- what shows a piece of engine state that a snapshot forgets;
  * pinned cases: the rules, one short list each;
  * the query layer (make_ops(queries=True)): behind every call zero to two read-only calls -- state_key, obs_key, action_mask,
    distance_field / agent_distance, the same on a kept snapshot, a key table, a selection.  The list without them is the list of
    queries=False, arguments included (the sub-list test: every failure name and census figure from before the layer stays valid);
    a query leaves every byte of env state, engine state, kept snapshots, the marker and its host flag alone (the fingerprint);
    a row query's answer is what the launcher gives on the rows it should have read -- the live `_cells` / agents / ... or the
    snapshot's own tensors --, asked for directly (two envs that share a fault of the host logic agree with each other).
  * the hook forms (es.HOOK_FORMS: RedBlueDoors, LockedHallway, Playground's generator, the declared rules): the same four tests,
    with a census of their own (es.HOOK_NEED, es.HOOK_QUERY_NEED) -- hook successes and failures, aux rewritten by a step, a restore
    and a fork that wrote another aux, generated restarts that carry one, steps with a visiting order while the marker is armed and
    while the accounting runs, outcomes the order decided, state keys that differ by hook state only, masks of a stale door -- and
    two checks in es.apply() that two envs sharing a fault cannot give each other: every launch a stepping call stands for received
    its visiting order, and a pool call installed the aux it was given.
tests/test_env_sequences_gpu.py runs the same lists on the HIP backend against this oracle.

Recorded host-logic mutants of multigrid_amd/batched.py for the hook forms (none committed, all in bounds), this file run once against
each (126 tests: the form lh12_pool came after these runs; no GPU run):

  (a) `snapshot()` leaves `aux` out of the members it copies (the snapshot keeps zeros).
      Dies: 6 failed, 120 passed.  The time machine of bup_candidates, rbd_candidates, lh_candidates, lh_pool and rules_pool (the
      repeated stretch differs: a state key, a termination, a reward) and the pinned case restore_of_a_changed_aux ("aux of the
      restored envs").  Every sequence and census case passes, as they must: both envs forget the same bytes.  rbd_pool's time
      machine passed (why was not looked into); the pinned case is RedBlueDoors'.
  (b) the adoption has no aux to copy: the candidate slots (`_gen["stage"]["aux"]`) are not made.
      Dies, but only by the assertion of es.make_env that the slots of rbd_candidates and lh_candidates hold an aux (13 failed: every
      test of these two forms and the pinned case reset_between_launch_and_adoption).  What the mutant is about cannot show here:
      the oracle generates in place and adopts nothing.  It is tests/test_env_sequences_gpu.py that holds the adopted aux to the
      oracle's, byte for byte after every call (not run against the mutant).
  (c) the slow path of `step` drops `hook_order` when sub_shards > 1 or while the marker is armed.
      As the driver stood first: SURVIVED, the 47 tests of the hook forms and the pinned cases passed -- both envs drop the same
      order, and the census counts calls, not what a launch received.  es.apply() now counts the launches that got a visiting
      order against those the call stands for, and kills it: 10 failed -- the sequences of rbd_pool (4 of 4) and lh_pool (2 of 4: the
      lists that step with an order while a one-layout pool has the marker armed), their census and time machine ("0 launch(es) got
      the visiting order, 1 stand for the call"; split(): 2 of 3).
  (d) `set_layout_pool` ignores `auxs` on an in-place refill.
      As the driver stood first: SURVIVED, the same 47 passed, census included -- the old pool's aux are hook-dense too.  es.apply()
      now holds the pool to the layouts, agent rows and aux of the call, and kills it: 18 failed, every sequence, census and time
      machine case of rbd_pool, lh_pool and rules_pool, at their first pool_refill."""
import functools

import numpy as np
import pytest
import torch

from multigrid_amd import _lib
from multigrid_amd.row_queries import _dist_query
from tests import env_sequences as es

SEQUENCES = [(130, 1), (130, 2), (130, 3), (7, 4)]            # (B, seed): what the census of a form is taken over
N_OPS = 120


def fingerprint(env, ctx) -> dict:
    """every byte a query must leave alone: what host_state() collects, the layout marker and its host flag"""
    d = {k: v.tobytes() for k, v in es.host_state(env, ctx).items()}
    d["_marker"], d["armed"] = env._marker.numpy().tobytes(), bool(env._mark["armed"])
    return d


def asked_directly(env, op, ctx) -> torch.Tensor:
    """The answer of a row query from the launcher itself, over the tensors the query should have read: none of `_copy_entry`,
    `_row_set` and row_queries.py in between."""
    be, sp = env.backend, env.spec
    if op["kind"] == "q_snap":
        which, snap = op["which"], ctx["snaps"][op["slot"]]
        t, n_rows = snap.tensors, snap.rows
    else:
        which, n_rows = es.WHICH[op["kind"]], env.batch
        t = {"cells": env._cells, "agents": env.agents, "rng": env.rng, "step_count": env.step_count, "aux": env.aux}
    idx = None if op["ids"] is None else torch.from_numpy(op["ids"])
    n = n_rows if idx is None else len(idx)
    if which == "key":
        keys = torch.zeros(n, dtype=torch.int64)
        flags = (_lib.KEY_STEP_COUNT if op["step_count"] else 0) | (_lib.KEY_RNG if op["rng"] else 0)
        be.state_key(n, {m: t.get(m) for m in ("cells", "agents", "rng", "step_count", "aux")}, n_rows, idx, flags, op["salt"], keys, None)
        return keys
    if which == "mask":
        mask = torch.zeros((n, sp.num_agents, 7), dtype=torch.bool) if op["expand"] else torch.zeros((n, sp.num_agents), dtype=torch.uint8)
        be.action_mask(n, {m: t.get(m) for m in ("cells", "agents", "aux")}, n_rows, idx, _lib.MASK_EXPAND if op["expand"] else 0, mask, None)
        return mask
    q = _dist_query("direct", sp, n, torch.device("cpu"), types=op["types"], colors=op["colors"], agents=op["agents"],
                    points=None if op["points"] is None else torch.from_numpy(op["points"]), through=op["through"],
                    avoid_lava=op["avoid_lava"])
    res = torch.full((n, sp.height, sp.width) if op["field"] else (n, sp.num_agents), -1, dtype=torch.int16)
    be.distance(n, {m: t.get(m) for m in ("cells", "agents")}, n_rows, idx, q, res if op["field"] else None, None if op["field"] else res, None)
    return res


@functools.lru_cache(maxsize=None)
def sequence(form, B, seed):
    """One list on two envs in lockstep; returns (the list, the first env's launcher)."""
    ops = es.make_ops(form, B, N_OPS, seed, queries=True)
    assert [es.describe(o) for o in es.make_ops(form, B, N_OPS, seed, queries=True)] == [es.describe(o) for o in ops], \
        "the list is not a function of its seed"
    a, b = es.make_env(form, B), es.make_env(form, B)
    ca, cb = es.new_ctx(), es.new_ctx()
    for i, op in enumerate(ops):
        where = es.where_text(form, B, seed, i, ops)
        query = op["kind"] in es.QUERY_KINDS
        before = fingerprint(a, ca) if query else None
        oa, ob_ = es.apply(a, op, ca, es.following(ops, i)), es.apply(b, op, cb, es.following(ops, i))
        if query:
            after = fingerprint(a, ca)
            changed = [k for k in before if before[k] != after[k]]
            assert not changed and set(before) == set(after), f"{where}: a query wrote {changed or sorted(set(before) ^ set(after))}"
        if op["kind"] in es.ROW_QUERIES + ("q_snap",):
            (got,) = [v for k, v in oa.items() if k.startswith("out.")]
            want = asked_directly(a, op, ca)
            assert got.dtype is want.dtype and got.numpy().tobytes() == want.numpy().tobytes(), \
                f"{where}: not the answer of the rows it names: {es.first_difference(want.numpy(), got.numpy())}"
        for env in (a, b):
            es.invariants(env, where)
            es.check_shadow(env, where)
        es.compare(a, b, ca, cb, where, oa, ob_)
    return ops, a.backend


@pytest.mark.parametrize("B,seed", SEQUENCES)
@pytest.mark.parametrize("form", es.FORMS + es.JIT_FORMS)
def test_a_sequence_keeps_the_invariants_and_repeats(form, B, seed):
    ops, be = sequence(form, B, seed)
    assert len(es.without_queries(ops)) == N_OPS
    assert not set(o["kind"] for o in ops) & set(es.GPU_KINDS + es.GPU_QUERY_KINDS)


def same_call(x, y) -> bool:
    """two calls of a list: the same kind and the same arguments, value for value"""
    def same(u, v):
        if isinstance(u, np.ndarray) or isinstance(v, np.ndarray):
            return isinstance(u, np.ndarray) and isinstance(v, np.ndarray) and u.dtype == v.dtype and u.shape == v.shape \
                and u.tobytes() == v.tobytes()
        return type(u) is type(v) and u == v
    return list(x) == list(y) and all(same(x[k], y[k]) for k in x)


#: every (B, seed, n_ops, gpu, stretch?) that a sequence test of the CPU or the GPU file draws a list with
GPU_SEQUENCES = [(130, 1), (130, 2), (7, 4)]


@pytest.mark.parametrize("form", es.FORMS + es.JIT_FORMS)
def test_the_list_without_its_queries_is_the_list_there_was(form):
    """make_ops(queries=True) with the query kinds filtered out equals make_ops(queries=False), arguments included -- for the lists of
    this file, of tests/test_env_sequences_gpu.py (the GPU kinds in) and of both time machines: the queries' draws come from a
    generator of their own, and n_ops counts the other calls."""
    cases = [(B, seed, N_OPS, False, None) for B, seed in SEQUENCES] + [(B, seed, N_OPS, True, None) for B, seed in GPU_SEQUENCES]
    cases += [(130, 5, s + n + 1, gpu, (s, s + n + 1)) for gpu in (False, True) for s, n in [time_machine_span(5)]]
    for B, seed, n_ops, gpu, stretch in cases:
        old = es.make_ops(form, B, n_ops, seed, gpu=gpu, stretch=stretch)
        new = es.make_ops(form, B, n_ops, seed, gpu=gpu, stretch=stretch, queries=True)
        kept = es.without_queries(new)
        assert len(old) == len(kept) == n_ops and len(new) > n_ops, (B, seed, gpu)
        for i, (x, y) in enumerate(zip(old, kept)):
            assert same_call(x, y), f"form {form} B={B} seed {seed} gpu={gpu}: call {i}: {es.describe(x)} became {es.describe(y)}"
        for i, op in enumerate(new):                          # the shape of the layer itself
            if op["kind"] in es.QUERY_KINDS:
                n = 0 if op.get("ids") is None else len(op["ids"])
                assert n <= es.MAX_QUERY_ROWS or B <= es.MAX_QUERY_ROWS
                assert not op.get("first_consumer") or (new[i - 1]["kind"] == "step_chains" and op["kind"] in es.FIRST_CONSUMERS)
            assert sum(o["kind"] in es.QUERY_KINDS for o in new[i:i + 3]) <= 2 or new[i]["kind"] not in es.QUERY_KINDS
        if stretch is not None:
            s = [o["kind"] for o in new].index("tm_begin")
            assert {o["kind"] for o in new[s + 1:]} <= set(es.PURE_KINDS)


@pytest.mark.parametrize("form", es.BIG_FORMS)
def test_the_large_list_without_its_queries_is_the_list_there_was(form):
    """the same for the lists of the size that reads the marker (tests/test_env_sequences_gpu.py: BIG_KINDS, BIG_WEIGHTS)"""
    from tests.test_env_sequences_gpu import BIG_KINDS, BIG_WEIGHTS, BIG_QUERY_KINDS
    from tests.test_grid_layout_marker import THROUGHPUT
    for seed in (1, 2):
        old = es.make_ops(form, THROUGHPUT, 40, seed, gpu=True, kinds=tuple(k for k in BIG_KINDS if k not in BIG_QUERY_KINDS),
                          weights={k: v for k, v in BIG_WEIGHTS.items() if k not in BIG_QUERY_KINDS}, every_third=True)
        new = es.make_ops(form, THROUGHPUT, 40, seed, gpu=True, kinds=BIG_KINDS, weights=BIG_WEIGHTS, every_third=True, queries=True)
        kept = es.without_queries(new)
        assert len(old) == len(kept) == 40 and len(new) > 40
        assert all(same_call(x, y) for x, y in zip(old, kept)), f"form {form} seed {seed}"
        for j, op in enumerate(new):
            if op["kind"] in es.QUERY_KINDS:
                assert op["kind"] in BIG_QUERY_KINDS
                if op["kind"] == "q_snap" and op["ids"] is None:          # (every row of a snapshot of at most 40 envs)
                    taken = [o for o in new[:j] if o["kind"] in ("snapshot", "snapshot_out") and o["slot"] == op["slot"]][-1]
                    assert taken["env_ids"] is not None and len(taken["env_ids"]) <= 40
                elif op["kind"] != "q_select":
                    assert op["ids"] is not None and len(op["ids"]) <= es.MAX_QUERY_ROWS <= 40


@pytest.mark.parametrize("form", es.FORMS + es.JIT_FORMS)
def test_census(form):
    runs = [sequence(form, B, seed) for B, seed in SEQUENCES]
    c = es.census_of([r[0] for r in runs], [r[1] for r in runs])
    es.assert_census(c, form, 130, queries=True)


# ---- the time machine ---------------------------------------------------------------------------------------------------------------

def time_machine_span(seed):
    """(s, n): the snapshot is call s of the list without its queries, n calls follow"""
    r = np.random.default_rng([seed, 77])
    return int(r.integers(15, 40)), int(r.integers(30, 61))


def time_machine(form, B, seed, device="cpu", gpu=False):
    """snapshot() of the whole batch at a random point, 30..60 calls, restore(), the same calls again"""
    s, n = time_machine_span(seed)
    ops = es.make_ops(form, B, s + n + 1, seed, gpu=gpu, stretch=(s, s + n + 1), queries=True)
    s = [o["kind"] for o in ops].index("tm_begin")           # (the query layer moved it: n still counts the other calls)
    env, ctx = es.make_env(form, B, device), es.new_ctx()
    host = lambda outs: {k: t.detach().cpu().numpy().copy() for k, t in outs.items()}
    recorded = []
    for i, op in enumerate(ops):
        outs = es.apply(env, op, ctx, es.following(ops, i))
        where = es.where_text(form, B, seed, i, ops)
        if not es.unjoined(op, es.following(ops, i)):        # (chains left to the query behind them: nothing reads the env before it)
            es.invariants(env, where)
        es.check_shadow(env, where)
        if i > s:
            recorded.append(host(outs))
    assert ops[s]["kind"] == "tm_begin" and len(es.without_queries(ops[s + 1:])) == n and len(recorded) == len(ops) - s - 1
    first = es.host_state(env, ctx)
    env.restore(ctx["tm"])
    ctx["snaps"] = {}
    be = env.backend
    if isinstance(be, es.SeqOracle) and be.shadow is not None:       # (the totals are no part of a snapshot: only the trio goes back)
        for m in es.TRIO:
            assert be.shadow[m].tobytes() == env._stats.tensors[m].numpy().tobytes()
    for j, op in enumerate(ops[s + 1:]):
        i = s + 1 + j
        where = "the second time: " + es.where_text(form, B, seed, i, ops)
        got = host(es.apply(env, op, ctx, es.following(ops, i)))
        if not es.unjoined(op, es.following(ops, i)):
            es.invariants(env, where)
        assert set(got) == set(recorded[j]), where
        for k in got:
            if got[k].tobytes() != recorded[j][k].tobytes():
                raise AssertionError(f"{where}: {k}: {es.first_difference(recorded[j][k], got[k], 1 if k.startswith('out.') else 0)}")
    totals = ("stats.last_return", "stats.last_length", "stats.sum_return", "stats.sum_length", "stats.counts")
    es.assert_same_state(first, es.host_state(env, ctx), f"form {form} B={B} seed {seed}: the state after the repeated stretch",
                         only=lambda k: k not in totals)
    env.check_errors()
    return ops[s + 1:]


@pytest.mark.parametrize("form", es.FORMS + es.JIT_FORMS)
def test_time_machine(form):
    kinds = {o["kind"] for o in time_machine(form, 130, 5)}
    assert kinds <= set(es.PURE_KINDS) and "step" in kinds and "restore" in kinds


# ---- pinned cases -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(es.PINNED))
def test_pinned(name):
    case = es.PINNED[name]()
    form, B, ops = case["form"], case["B"], case["ops"]
    a, b = es.make_env(form, B), es.make_env(form, B)
    ca, cb = es.new_ctx(), es.new_ctx()
    for i, op in enumerate(ops):
        where = f"pinned case {name}: call {i}: {es.describe(op)}"
        oa, ob_ = es.apply(a, op, ca), es.apply(b, op, cb)
        for env in (a, b):
            es.invariants(env, where)
            es.check_shadow(env, where)
        es.compare(a, b, ca, cb, where, oa, ob_)
        if i in case.get("checks", {}):
            case["checks"][i](a, where)
