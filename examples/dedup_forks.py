#!/usr/bin/env python3
"""Search roll-outs without duplicate work: fork a few root envs over the batch, let every fork try its own actions, and dedup the
states they reach with `torch.unique(env.state_key())` -- the transposition table of a search, the cell key of a Go-Explore
archive.  Everything stays on the device: fork() is two launches, state_key() one.

    python examples/dedup_forks.py [--workload c2] [--roots 8] [--depth 3]

Prints one JSON line: how many of the batch's envs hold a state nobody else holds, level by level."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigrid_amd import workloads  # noqa: E402


def run(workload="c2", roots=8, depth=3, device="cuda:0"):
    dev = torch.device(device)
    wl = workloads.make(workload)
    env = wl.make_env(dev, auto_reset=False)
    B, A = wl.batch, wl.spec.num_agents
    g = torch.Generator(device=dev); g.manual_seed(0)
    act = lambda: torch.randint(0, 3, (B, A), dtype=torch.int8, device=dev, generator=g)      # left / right / forward
    for _ in range(4):                                                       # the roots part from each other first
        env.step(act())
    # every env of the batch becomes a fork of one of the first `roots` envs
    dst = torch.arange(roots, B, device=dev)
    env.fork(dst % roots, dst)
    levels = [int(torch.unique(env.state_key()).numel())]
    assert levels[0] <= roots
    for _ in range(depth):
        env.step(act())
        keys = env.state_key()                                               # int64 [B]; np_random is not part of it (rng=False)
        uniq, inverse = torch.unique(keys, return_inverse=True)
        levels.append(int(uniq.numel()))
        # keep ONE env per distinct state and refill the rest of the batch with forks of the kept ones
        first = torch.full((uniq.numel(),), B, dtype=torch.int64, device=dev).scatter_reduce_(0, inverse, torch.arange(B, device=dev),
                                                                                               reduce="amin")
        keep = torch.zeros(B, dtype=torch.bool, device=dev)
        keep[first] = True
        free = torch.nonzero(~keep).flatten()
        if free.numel():
            env.fork(first[torch.arange(free.numel(), device=dev) % first.numel()].contiguous(), free.contiguous())
    env.check_errors()
    return {"workload": wl.title, "batch": B, "roots": roots, "distinct_states_per_level": levels}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--roots", type=int, default=8)
    ap.add_argument("--depth", type=int, default=3)
    a = ap.parse_args()
    print(json.dumps(run(a.workload, a.roots, a.depth)))
