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
  * pinned cases: the rules, one short list each.
tests/test_env_sequences_gpu.py runs the same lists on the HIP backend against this oracle."""
import functools

import numpy as np
import pytest
import torch

from tests import env_sequences as es

SEQUENCES = [(130, 1), (130, 2), (130, 3), (7, 4)]            # (B, seed): what the census of a form is taken over
N_OPS = 120


@functools.lru_cache(maxsize=None)
def sequence(form, B, seed):
    """One list on two envs in lockstep; returns (the list, the first env's launcher)."""
    ops = es.make_ops(form, B, N_OPS, seed)
    assert [es.describe(o) for o in es.make_ops(form, B, N_OPS, seed)] == [es.describe(o) for o in ops], "the list is not a function of its seed"
    a, b = es.make_env(form, B), es.make_env(form, B)
    ca, cb = es.new_ctx(), es.new_ctx()
    for i, op in enumerate(ops):
        where = es.where_text(form, B, seed, i, ops)
        oa, ob_ = es.apply(a, op, ca), es.apply(b, op, cb)
        for env in (a, b):
            es.invariants(env, where)
            es.check_shadow(env, where)
        es.compare(a, b, ca, cb, where, oa, ob_)
    return ops, a.backend


@pytest.mark.parametrize("B,seed", SEQUENCES)
@pytest.mark.parametrize("form", es.FORMS + es.JIT_FORMS)
def test_a_sequence_keeps_the_invariants_and_repeats(form, B, seed):
    ops, be = sequence(form, B, seed)
    assert len(ops) == N_OPS
    assert not set(o["kind"] for o in ops) & set(es.GPU_KINDS)


@pytest.mark.parametrize("form", es.FORMS + es.JIT_FORMS)
def test_census(form):
    runs = [sequence(form, B, seed) for B, seed in SEQUENCES]
    c = es.census_of([r[0] for r in runs], [r[1] for r in runs])
    es.assert_census(c, form, 130)


# ---- the time machine ---------------------------------------------------------------------------------------------------------------

def time_machine(form, B, seed, device="cpu", gpu=False):
    """snapshot() of the whole batch at a random point, 30..60 calls, restore(), the same calls again"""
    r = np.random.default_rng([seed, 77])
    s, n = int(r.integers(15, 40)), int(r.integers(30, 61))
    ops = es.make_ops(form, B, s + n + 1, seed, gpu=gpu, stretch=(s, s + n + 1))
    env, ctx = es.make_env(form, B, device), es.new_ctx()
    host = lambda outs: {k: t.detach().cpu().numpy().copy() for k, t in outs.items()}
    recorded = []
    for i, op in enumerate(ops):
        outs = es.apply(env, op, ctx)
        where = es.where_text(form, B, seed, i, ops)
        es.invariants(env, where)
        es.check_shadow(env, where)
        if i > s:
            recorded.append(host(outs))
    assert ops[s]["kind"] == "tm_begin" and len(recorded) == n
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
        got = host(es.apply(env, op, ctx))
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
