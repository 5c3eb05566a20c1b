"""The hook-dense cases of tests/hook_states.py are not hollow, and the g++ build of mgx_rules.h agrees with the oracle on them.

Counted on the CPU oracle alone: for every case, the number of envs (of 512) that reach each class of hook event at least once.
Every class must be reached by at least FLOOR envs -- a condition on the INPUTS (the builder's placements and action weights), not
a measurement of any kernel: the GPU tests of tests/test_hook_kinds_gpu.py rely on it for their density and do not count again.
Where the visiting order can change a result (hook_states.CASES), the run with ascending order must differ from the scripted one in
at least FLOOR envs; where it provably cannot, the two runs must be identical.

Then tests/hostshim (mgx_rules.h compiled by g++) steps the cases env by env on 16-bit and on compact cells, with the order-free path
and the sequential one, against the oracle: every output and the whole post-step state, aux included."""
import dataclasses

import numpy as np
import pytest

from tests import hook_states as hs
from tests import hostshim

FLOOR = 32
DX, DY = np.array([1, 0, -1, 0]), np.array([0, 1, 0, -1])


def _front(agents):
    d = agents[..., 1] & 3
    return agents[..., 2].astype(np.int64) + DX[d], agents[..., 3].astype(np.int64) + DY[d]


def _steps(name):
    """(pre-state, actions, record of the step) for every step of the case's oracle run"""
    c = hs.case(name)
    traj = hs.trajectory(name)
    pre = c.state
    for t, rec in enumerate(traj):
        yield pre, c.actions[t], rec
        pre = rec


def _rv(pre, spec):
    return 1 - 0.9 * ((pre["step_count"] + 1).astype(np.float64) / spec.max_steps)


def count_redbluedoors(name):
    c = hs.case(name)
    g0, a0 = c.state["grid"], c.state["aux"]
    b = np.arange(hs.BASE)
    blue0, red0 = g0[b, a0[:, 1], a0[:, 0], 2], g0[b, a0[:, 3], a0[:, 2], 2]
    ev = {"start_both_closed": (blue0 == hs.CLOSED) & (red0 == hs.CLOSED), "start_red_open": (red0 == hs.OPEN) & (blue0 == hs.CLOSED)}
    for k in ("success", "failure_sets_stale", "unstale", "two_togglers_one_door", "truncated"):
        ev[k] = np.zeros(hs.BASE, bool)
    for pre, act, rec in _steps(name):
        fx, fy = _front(pre["agents"])
        live_tog = (act == hs.TOGGLE) & (pre["agents"][..., 4] == 0)
        at_blue = live_tog & (fx == pre["aux"][:, None, 0]) & (fy == pre["aux"][:, None, 1])
        at_red = live_tog & (fx == pre["aux"][:, None, 2]) & (fy == pre["aux"][:, None, 3])
        ev["success"] |= (rec["reward"] > 0).any(1)
        ev["failure_sets_stale"] |= (pre["aux"][:, 4] == 0) & (rec["aux"][:, 4] == 1)
        ev["unstale"] |= (pre["aux"][:, 4] == 1) & at_blue.any(1)
        ev["two_togglers_one_door"] |= (at_blue.sum(1) >= 2) | (at_red.sum(1) >= 2)
        ev["truncated"] |= rec["truncated"] != 0
    return ev


def _door_index(aux, fx, fy):
    """LockedHallway: the index of the door at (fx, fy) [B,A] in the env's aux, or -1 (mgx_rules.h: post_step_hook)"""
    B, A = fx.shape
    k = np.full((B, A), -1, np.int64)
    geo = (aux[:, 0] & 0x80) != 0
    nd = (aux[:, 0] & 0x7f).astype(np.int64)
    rs = aux[:, 3].astype(np.int64)
    for b in range(B):
        for a in range(A):
            if geo[b]:
                side = 1 if fx[b, a] == 2 * (rs[b] - 1) else (0 if fx[b, a] == rs[b] - 1 else -1)
                yy = fy[b, a] - (rs[b] - 1) // 2
                if side >= 0 and yy >= 0 and yy % (rs[b] - 1) == 0 and 2 * (yy // (rs[b] - 1)) + side < nd[b]:
                    k[b, a] = 2 * (yy // (rs[b] - 1)) + side
            else:
                for j in range(nd[b]):
                    if aux[b, 2 + 2 * j] == fx[b, a] and aux[b, 3 + 2 * j] == fy[b, a]:
                        k[b, a] = j
                        break
    return k


def count_lockedhallway(name):
    c = hs.case(name)
    geo = bool(c.state["aux"][0, 0] & 0x80)
    names = ["first_unlock", "repeated_toggle_unpaid", "two_agents_one_door_unlock", "unlock_with_goal_or_lava", "forced_termination",
             "truncated"]
    if c.spec.joint_reward:
        names.append("unlock_added_onto_base_reward")
    if geo and (c.state["aux"][0, 0] & 0x7f) > 8:
        names.append("unlock_in_second_mask_byte")
    ev = {k: np.zeros(hs.BASE, bool) for k in names}
    b = np.arange(hs.BASE)
    for pre, act, rec in _steps(name):
        mask0 = pre["aux"][:, 1].astype(np.int64) | ((pre["aux"][:, 2].astype(np.int64) << 8) if geo else 0)
        mask1 = rec["aux"][:, 1].astype(np.int64) | ((rec["aux"][:, 2].astype(np.int64) << 8) if geo else 0)
        gained = mask1 & ~mask0
        fx, fy = _front(rec["agents"])                               # (the hook looks at the rows after the step)
        k = _door_index(pre["aux"], fx, fy)
        tog = (act == hs.TOGGLE) & (k >= 0)
        kk = np.where(k >= 0, k, 0)
        on_old = tog & (((mask0[:, None] >> kk) & 1) == 1)
        on_new = tog & (((gained[:, None] >> kk) & 1) == 1)
        paid = (rec["reward"] > 0).any(1)
        ev["first_unlock"] |= (gained != 0) & paid
        ev["repeated_toggle_unpaid"] |= on_old.any(1) & (gained == 0) & ~paid
        two = np.zeros(hs.BASE, bool)
        for a in range(c.spec.num_agents):
            for a2 in range(a):
                two |= on_new[:, a] & on_new[:, a2] & (k[:, a] == k[:, a2])
        ev["two_agents_one_door_unlock"] |= two
        moved = (act == hs.FORWARD) & (pre["agents"][..., 4] == 0) & ((pre["agents"][..., 2:4] != rec["agents"][..., 2:4]).any(-1))
        cell = rec["grid"][b[:, None], rec["agents"][..., 3], rec["agents"][..., 2], 0]
        base = (moved & ((cell == hs.GOAL) | (cell == hs.LAVA))).any(1)
        ev["unlock_with_goal_or_lava"] |= (gained != 0) & base
        if "unlock_added_onto_base_reward" in ev:
            ev["unlock_added_onto_base_reward"] |= (gained != 0) & (rec["reward"] > 1.5 * _rv(pre, c.spec)[:, None]).any(1)
        ev["forced_termination"] |= (pre["aux"][:, 15] == 0) & (rec["aux"][:, 15] == 1)
        if "unlock_in_second_mask_byte" in ev:
            ev["unlock_in_second_mask_byte"] |= (gained >> 8) != 0
        ev["truncated"] |= rec["truncated"] != 0
    return ev


def count_rules(name):
    c = hs.case(name)
    aux = c.state["aux"]
    want = aux[:, 2].astype(np.int64) | (aux[:, 3].astype(np.int64) << 8)             # rule 0: carries (type, colour)
    has_toggle = bool(aux[0, 0] > 1)
    names = ["carries_succeeds", "carries_fails", "truncated"] + (["toggles_at_succeeds", "toggles_at_door_ends_shut", "toggles_elsewhere"] if has_toggle else [])
    ev = {k: np.zeros(hs.BASE, bool) for k in names}
    b = np.arange(hs.BASE)
    for pre, act, rec in _steps(name):
        carry = rec["agents"][..., 5].astype(np.int64) | (rec["agents"][..., 6].astype(np.int64) << 8)
        ev["carries_succeeds"] |= ((carry == want[:, None]) & (rec["reward"] > 0)).any(1)
        ev["carries_fails"] |= ((rec["agents"][..., 5] != 1) & (carry != want[:, None])).any(1)
        ev["truncated"] |= rec["truncated"] != 0
        if has_toggle:
            fx, fy = _front(rec["agents"])
            tog = act == hs.TOGGLE
            at = tog & (fx == aux[:, None, 7]) & (fy == aux[:, None, 8])
            door_open = rec["grid"][b, aux[:, 8], aux[:, 7], 2] == hs.OPEN
            newly = (pre["agents"][..., 4] == 0) & (rec["agents"][..., 4] != 0) & ~(rec["reward"] > 0)
            ev["toggles_at_succeeds"] |= (at & door_open[:, None] & newly).any(1)
            ev["toggles_at_door_ends_shut"] |= (at & ~door_open[:, None]).any(1)          # at the named cell, the condition fails
            ev["toggles_elsewhere"] |= (tog & ~at).any(1)                                 # the position test fails
    return ev


COUNTERS = {"redbluedoors": count_redbluedoors, "lockedhallway": count_lockedhallway, "rules": count_rules}


@pytest.mark.parametrize("name", hs.NAMES)
def test_every_event_class_is_reached_by_at_least_32_envs(name):
    c = hs.case(name)
    assert c.state["grid"].shape[0] == hs.BASE == 512
    ev = COUNTERS[hs.kind_of(name)](name)
    counts = {k: int(v.sum()) for k, v in ev.items()}
    print(name, counts)
    low = {k: n for k, n in counts.items() if n < FLOOR}
    assert not low, f"{name}: event classes reached by fewer than {FLOOR} of {hs.BASE} envs: {low} (all: {counts})"


@pytest.mark.parametrize("name", [n for n in hs.NAMES if hs.kind_of(n) != "rules"])
def test_the_visiting_order_matters_in_at_least_32_envs(name):
    c = hs.case(name)
    assert c.hook_order is not None
    differs = np.zeros(hs.BASE, bool)
    for x, y in zip(hs.trajectory(name, True), hs.trajectory(name, False)):
        differs |= (x["reward"].view(np.int64) != y["reward"].view(np.int64)).any(1) | (x["terminated"] != y["terminated"]).any(1)
    print(name, "envs where the visiting order changes a reward or a termination:", int(differs.sum()))
    if c.order_can_matter:
        assert differs.sum() >= FLOOR, f"{name}: the visiting order matters in {int(differs.sum())} envs only"
    else:
        # symmetric by construction of the hook (hook_states.CASES): RedBlueDoors under failure mode "any", LockedHallway with a joint
        # reward -- whoever is visited first, the same agents end and the same agents are paid
        assert not differs.any(), f"{name}: the visiting order changed a result where the hook is symmetric in it"


HOST_ENVS = 60          # (a multiple of every kind's number of scenarios: env b starts in scenario b % n)


@pytest.mark.parametrize("force_serial", [False, True], ids=["fastpath", "serial"])
@pytest.mark.parametrize("cell_bytes", [2, 1], ids=["cells16", "compact"])
@pytest.mark.parametrize("name", hs.NAMES)
def test_host_rules_match_the_oracle_on_hook_dense_states(name, cell_bytes, force_serial):
    c = hs.case(name)
    spec = dataclasses.replace(c.spec, cell_bytes=cell_bytes)
    traj = hs.trajectory(name)
    st = {k: v[:HOST_ENVS].copy() for k, v in c.state.items()}
    for t, rec in enumerate(traj):
        for b in range(HOST_ENVS):
            out = hostshim.step_env(spec, st["grid"][b], st["agents"][b], np.ascontiguousarray(c.actions[t, b]), st["rng"][b],
                                    st["step_count"][b], st["aux"][b], force_serial,
                                    hook_order=None if c.hook_order is None else c.hook_order[t, b])
            st["step_count"][b] = out["step_count"]
            ctx = f"{name} step {t} env {b} (scenario {c.scenario[b]})"
            assert out["rc"] == 0, ctx
            np.testing.assert_array_equal(out["obs"], rec["obs"][b], err_msg=ctx)
            np.testing.assert_array_equal(st["agents"][b][:, 1], rec["dir"][b], err_msg=ctx)   # (the shim hands back no `dir`: the rows')
            assert out["reward"].tobytes() == rec["reward"][b].tobytes(), ctx
            np.testing.assert_array_equal(out["terminated"], rec["terminated"][b], err_msg=ctx)
            assert out["truncated"] == rec["truncated"][b], ctx
        for k in ("grid", "agents", "rng", "step_count", "aux"):
            np.testing.assert_array_equal(st[k], rec[k][:HOST_ENVS], err_msg=f"{name} step {t}: {k}")
