#!/usr/bin/env python3
"""Expand a search frontier without forking children that cannot differ: `env.action_mask()` says which of an agent's actions do
anything in the state it is in, so only those children are forked and stepped; the rest equal the child that takes `done`, which
the parent itself plays.  The children are then deduplicated by `torch.unique(env.state_key())`, as examples/dedup_forks.py does
after paying for all 7 of them.  Everything stays on the device: action_mask() is one launch, fork() two, state_key() one.

    python examples/masked_expand.py [--workload c3] [--roots 8] [--depth 4] [--no-verify]

The frontier lives in the first envs of the batch; agent 0 searches, the other agents play `done`.  With --verify (the default) every
level is also expanded 7 ways from the same frontier, and the two expansions must reach the same set of states: a clear bit is a
promise.  Prints one JSON line: the frontier level by level, the forks made and the forks a 7-way expansion makes."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigrid_amd import workloads  # noqa: E402

DONE, ACTIONS = 6, 7


def expand(env, F, parent, action):
    """fork env parent[i] into env F + i and let its agent 0 take action[i] there; the envs [0, F) play `done` (each is its own
    seventh child); one step.  Returns the state keys of the F + n envs."""
    dev, n = parent.device, int(parent.numel())
    dst = torch.arange(F, F + n, device=dev)
    if n:
        env.fork(parent.contiguous(), dst)
    act = torch.full((env.batch, env.spec.num_agents), DONE, dtype=torch.int8, device=dev)
    act[dst, 0] = action.to(torch.int8)
    env.step(act)
    return env.state_key(torch.arange(F + n, device=dev))


def run(workload="c3", roots=8, depth=4, batch=None, device="cuda:0", verify=True, backend=None):
    dev = torch.device(device)
    wl = workloads.make(workload, batch=batch)
    env = wl.make_env(dev, auto_reset=False, **({"backend": backend} if backend is not None else {}))
    B = wl.batch
    cap = B // ACTIONS                                                        # a frontier that can still be expanded 7 ways
    F = min(roots, cap)
    six = torch.arange(ACTIONS - 1, device=dev)
    frontier, forks, forks_7way = [F], 0, 0
    for _ in range(depth):
        ids = torch.arange(F, device=dev)
        if verify:                                                           # all six other children of every frontier env
            snap = env.snapshot()
            reached_7way = torch.unique(expand(env, F, ids.repeat_interleave(ACTIONS - 1), six.repeat(F)))
            env.restore(snap)
        mask = env.action_mask(ids)                                          # uint8 [F, A]: bit k = action k of that agent
        parent, action = torch.nonzero((mask[:, :1] >> six) & 1, as_tuple=True)
        keys = expand(env, F, parent, action)
        forks += int(parent.numel())
        forks_7way += (ACTIONS - 1) * F
        uniq, inverse = torch.unique(keys, return_inverse=True)
        if verify:
            assert torch.equal(uniq, reached_7way), "the masked expansion reached other states than the 7-way expansion"
        # keep ONE env per distinct state and move the kept ones to the front: the next frontier
        first = torch.full((uniq.numel(),), B, dtype=torch.int64, device=dev).scatter_reduce_(
            0, inverse, torch.arange(keys.numel(), device=dev), reduce="amin")[:cap]
        F = int(first.numel())
        env.fork(first.contiguous(), torch.arange(F, device=dev))
        frontier.append(F)
    env.check_errors()
    return {"workload": wl.title, "batch": B, "frontier_per_level": frontier, "forks": forks, "forks_7way": forks_7way,
            "forks_saved": round(1.0 - forks / max(1, forks_7way), 3), "verified": bool(verify)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--roots", type=int, default=8)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--no-verify", action="store_true")
    a = ap.parse_args()
    print(json.dumps(run(a.workload, a.roots, a.depth, verify=not a.no_verify)))
