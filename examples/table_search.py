#!/usr/bin/env python3
"""Best-first search with the visited set on the device: the expansion loop of examples/best_first.py -- fork only the children
`action_mask()` says can differ, step, key with `state_key()` -- where a `KeyTable` takes the place of `torch.unique` / `torch.isin` /
`torch.cat`.  One `table.insert(keys)` answers, for the whole level, "which of these states has nobody seen, and which env holds each
first": the children are `dst[is_new]`.  The table's memory is constant; the torch formulation re-scans everything seen so far at
every level and synchronises with the host for `unique`'s output size.

The ENTRY ID the table gives every state indexes a tensor of the caller's: here `depth_of[entry]`, the level at which a state was
first reached, which orders the frontier together with `agent_distance()` (depth + the moves agent 0 still has to make).

    python examples/table_search.py [--workload c2] [--beam 8] [--depth 40] [--capacity 16384] [--check]

`--check` also computes, at every level, the new keys the torch formulation would choose and asserts that the table chose the same
set of keys, one env each, and each the smallest index that holds it.  Prints one JSON line; `drops` must be 0 (a table kept at a
load of a half or below drops nothing)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigrid_amd import workloads  # noqa: E402
from multigrid_amd.constants import Type  # noqa: E402

DONE, ACTIONS, FAR = 6, 7, 4096


def heuristic(env, ids):
    """int64 [n]: the moves agent 0 of the envs `ids` has to make at least; FAR when there is no way"""
    d = env.agent_distance(ids, types=[Type.goal])[:, 0].to(torch.int64)
    return torch.where(d < 0, torch.full_like(d, FAR), d)


def torch_choice(keys, seen):
    """what examples/best_first.py computes: (the indices of `keys` that hold a key not in `seen`, one per key, the smallest;
    for every index the smallest index with the same key)"""
    n, dev = keys.numel(), keys.device
    uniq, inverse = torch.unique(keys, return_inverse=True)
    first = torch.full((uniq.numel(),), n, dtype=torch.int64, device=dev).scatter_reduce_(
        0, inverse, torch.arange(n, device=dev), reduce="amin")
    return first[~torch.isin(uniq, seen)], first[inverse]


def search(env, table, roots, beam, depth, check=False):
    """expand level by level from the envs [0, roots); returns a dict of the nodes expanded, the depth reached, whether agent 0 of
    some env terminated, and per level the number of states nobody had seen"""
    dev, B = env.agents.device, env.batch
    cap = B // ACTIONS
    six = torch.arange(ACTIONS - 1, device=dev)
    F, expanded, found, reached, levels = min(roots, cap), 0, False, 0, []
    depth_of = torch.full((table.capacity,), -1, dtype=torch.int64, device=dev)       # per ENTRY: the level that first reached it
    keys = env.state_key(torch.arange(F, device=dev))
    res = table.insert(keys)
    depth_of[res.entry[res.is_new]] = 0
    seen = keys.clone() if check else None
    for level in range(1, depth + 1):
        reached = level
        ids = torch.arange(F, device=dev)
        mask = env.action_mask(ids)
        parent, action = torch.nonzero((mask[:, :1] >> six) & 1, as_tuple=True)
        n = int(parent.numel())
        expanded += F
        if n == 0:
            break
        dst = torch.arange(F, F + n, device=dev)
        env.fork(parent.contiguous(), dst)
        act = torch.full((B, env.spec.num_agents), DONE, dtype=torch.int8, device=dev)
        act[dst, 0] = action.to(torch.int8)
        env.step(act)
        if bool(env.agents[dst, 0, 4].any()):
            found = True
            break
        keys = env.state_key(dst)
        res = table.insert(keys, first=check)                                 # two launches: the whole level's dedup
        if check:
            want, want_first = torch_choice(keys, seen)
            got = torch.nonzero(res.is_new).squeeze(1)
            # the same indices: hence the same set of keys, one env each, and each the smallest index holding its key
            assert got.tolist() == sorted(want.tolist()), (level, got.tolist(), sorted(want.tolist()))
            assert torch.equal(res.first, want_first), level
            assert torch.equal(keys[got].sort().values, torch.unique(keys[got])), level
            seen = torch.cat((seen, keys[got]))
        new = res.is_new
        entry = res.entry[new]
        depth_of[entry] = level
        children = dst[new]
        levels.append(int(children.numel()))
        if children.numel() == 0:
            break
        order = torch.argsort(depth_of[entry] + heuristic(env, children.contiguous()), stable=True)
        children = children[order][:beam][:cap].contiguous()
        F = int(children.numel())
        env.fork(children, torch.arange(F, device=dev))
    return {"nodes_expanded": expanded, "depth": reached, "found": found, "new_per_level": levels}


def run(workload="c2", roots=1, beam=8, depth=40, batch=None, device="cuda:0", backend=None, capacity=1 << 14, check=False):
    dev = torch.device(device)
    wl = workloads.make(workload, batch=batch)
    if not (wl.grid[..., 0] == int(Type.goal)).any():
        raise ValueError(f"table_search: workload {workload} has no goal cell for the heuristic to aim at")
    env = wl.make_env(dev, auto_reset=False, **({"backend": backend} if backend is not None else {}))
    table = env.key_table(capacity)
    out = {"workload": wl.title, "batch": wl.batch, "roots": roots, "beam": beam, "capacity": capacity, "checked": bool(check)}
    out.update(search(env, table, roots, beam, depth, check))
    out["table_entries"], out["drops"] = table.entries(), table.dropped()
    assert out["table_entries"] == 1 + sum(out["new_per_level"]) or roots != 1, out
    env.check_errors()
    table.check_errors()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--roots", type=int, default=1)
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--depth", type=int, default=40)
    ap.add_argument("--capacity", type=int, default=1 << 14)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    print(json.dumps(run(a.workload, a.roots, a.beam, a.depth, capacity=a.capacity, check=a.check)))
