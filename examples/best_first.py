#!/usr/bin/env python3
"""Best-first search on the device: the expansion of examples/masked_expand.py -- fork only the children `action_mask()` says can
differ, step, dedup by `state_key()` -- with the frontier ORDERED by depth + `agent_distance()`, the number of moves agent 0 still
has to make, walls respected, and truncated to a beam.  The same roots are then searched breadth-first (the frontier in the order the
children come, truncated only by the room the batch has), and the two are compared by the nodes they expand until an env's agent 0
has terminated.  Everything stays on the device: agent_distance() is one launch.

    python examples/best_first.py [--workload c2] [--beam 8] [--depth 40]

The heuristic is the distance to the goal, so the workload must be one with a goal cell (the Empty workloads c2, c4).  Distances count
moves, turns are free: the heuristic never overestimates.  Prints one JSON line."""
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


def search(env, roots, beam, depth, informed):
    """expand level by level from the envs [0, roots); returns (nodes expanded, depth reached, whether agent 0 of some env terminated)"""
    dev, B = env.agents.device, env.batch
    cap = B // ACTIONS
    six = torch.arange(ACTIONS - 1, device=dev)
    F, expanded = min(roots, cap), 0
    seen = env.state_key(torch.arange(F, device=dev))
    for level in range(1, depth + 1):
        ids = torch.arange(F, device=dev)
        mask = env.action_mask(ids)
        parent, action = torch.nonzero((mask[:, :1] >> six) & 1, as_tuple=True)
        n = int(parent.numel())
        expanded += F
        if n == 0:
            return expanded, level, False
        dst = torch.arange(F, F + n, device=dev)
        env.fork(parent.contiguous(), dst)
        act = torch.full((B, env.spec.num_agents), DONE, dtype=torch.int8, device=dev)
        act[dst, 0] = action.to(torch.int8)
        env.step(act)
        if bool(env.agents[dst, 0, 4].any()):
            return expanded, level, True
        keys = env.state_key(dst)
        uniq, inverse = torch.unique(keys, return_inverse=True)
        first = torch.full((uniq.numel(),), B, dtype=torch.int64, device=dev).scatter_reduce_(
            0, inverse, torch.arange(n, device=dev), reduce="amin")
        first = first[~torch.isin(uniq, seen)] + F                            # one env per state nobody has expanded yet
        if first.numel() == 0:
            return expanded, level, False
        seen = torch.cat((seen, env.state_key(first.contiguous())))
        if informed:                                                          # every child has the same depth: order by what is left
            order = torch.argsort(heuristic(env, first.contiguous()), stable=True)
            first = first[order][:beam]
        first = first[:cap].contiguous()
        F = int(first.numel())
        env.fork(first, torch.arange(F, device=dev))
    return expanded, depth, False


def run(workload="c2", roots=1, beam=8, depth=40, batch=None, device="cuda:0", backend=None):
    dev = torch.device(device)
    wl = workloads.make(workload, batch=batch)
    if not (wl.grid[..., 0] == int(Type.goal)).any():
        raise ValueError(f"best_first: workload {workload} has no goal cell for the heuristic to aim at")
    env = wl.make_env(dev, auto_reset=False, **({"backend": backend} if backend is not None else {}))
    start = env.snapshot()
    out = {"workload": wl.title, "batch": wl.batch, "roots": roots, "beam": beam}
    for name, informed in (("best_first", True), ("breadth_first", False)):
        env.restore(start)
        nodes, reached, found = search(env, roots, beam, depth, informed)
        out[name] = {"nodes_expanded": nodes, "depth": reached, "found": bool(found)}
    env.check_errors()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--roots", type=int, default=1)
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--depth", type=int, default=40)
    a = ap.parse_args()
    print(json.dumps(run(a.workload, a.roots, a.beam, a.depth)))
