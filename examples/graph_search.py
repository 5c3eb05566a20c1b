#!/usr/bin/env python3
"""A whole search level as ONE captured graph: the beam search of examples/table_search.py in fixed shapes, so that nothing of a
level leaves the device -- no `nonzero`, no boolean indexing, no `argsort` of the level, no `int(numel())` -- and the host reads one
status tensor of four words per level.  What makes the shapes fixed is `Selector.select` (include/mgx.h "SELECTION"): "the k best of
these n, as a list of fixed length, with the count kept on the device".

LAYOUT, with cap = B // 7: the frontier lives in the rows [0, cap), child slot j is the row cap + j for j < 6 * cap, and F -- how
many frontier rows are in use -- is a device word.  A level:

    the masks of the frontier rows, those of the rows >= F cleared                                      action_mask
    select(keep=flags, k=6 * cap): the (parent, action) pairs in `nonzero` order                        two launches
    padded pairs fork row 0 and take `done`; one fork, one step                                          snapshot + restore, step
    over the child slots: state_key, table.insert(count=False), agent_distance                           -- a padded child equals row
      0's state, which the table already holds, so it is never new
    depth_of[entry] = level for the new entries; every other child writes the one sink slot behind the table's entries
    select(score=depth + distance, keep=is_new & valid, k=min(beam, cap), values=child rows, fill=0)    six launches: the next
      frontier and F
    one fork moves the chosen children into the frontier rows (a padded entry copies row 0 into a row >= F, which nobody reads)
    status = (level, F, found, new children of this level)

    python examples/graph_search.py [--workload c2] [--beam 8] [--depth 40] [--capacity 16384] [--graph | --check]

`--graph` captures the level once in a `torch.cuda.graph` and replays it; the level counter is a device word, so every replay is the
next level.  `--check` runs eagerly and compares, at every level, both selections with what torch computes from the same tensors:
`nonzero(flags)` and `sort(argsort(where(keep, score, BIG), stable=True)[:count])`.  Prints one JSON line.

The frontier is kept in ASCENDING CHILD INDEX, not in rank order as table_search.py keeps it, so the children of the next level are
numbered differently and ties at the beam's edge may fall to other states: the two programs search the same space with the same
heuristic, but their traces are not compared with each other."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigrid_amd import workloads  # noqa: E402
from multigrid_amd.constants import Type  # noqa: E402

DONE, ACTIONS, FAR, BIG = 6, 7, 4096, 1 << 40
LEVEL, FRONT, FOUND, CHILDREN = range(4)                   # the status words


class Level:
    """the tensors of a level, allocated once, and `run()`: one level, every shape fixed, nothing read by the host"""

    def __init__(self, env, table, beam, check=False):
        dev, B, A = env.agents.device, env.batch, env.spec.num_agents
        self.env, self.table, self.check = env, table, check
        self.cap = cap = B // ACTIONS
        self.slots = slots = (ACTIONS - 1) * cap
        self.beam = min(beam, cap)
        self.sel = env.selector(slots)
        self.front_ids = torch.arange(cap, device=dev)
        self.child_ids = torch.arange(cap, cap + slots, device=dev)
        self.six = torch.arange(ACTIONS - 1, device=dev, dtype=torch.uint8)
        self.status = torch.zeros(4, dtype=torch.int64, device=dev)
        self.mask = torch.zeros((cap, A), dtype=torch.uint8, device=dev)
        self.act = torch.full((B, A), DONE, dtype=torch.int8, device=dev)
        self.keys = torch.zeros(slots, dtype=torch.int64, device=dev)
        self.dist = torch.zeros((slots, A), dtype=torch.int16, device=dev)
        self.depth_of = torch.full((table.capacity + 1,), -1, dtype=torch.int64, device=dev)      # [capacity]: the sink
        self.pairs = self.nxt = self.res = self.snap_children = self.snap_front = None
        self.checked = 0

    def root(self, roots):
        """the envs [0, roots) are the first frontier"""
        F = min(roots, self.cap)
        res = self.table.insert(self.env.state_key(self.front_ids[:F].contiguous()))
        self.depth_of[res.entry[res.is_new]] = 0
        self.status[FRONT] = F

    def run(self):
        env, sel, st, cap, slots = self.env, self.sel, self.status, self.cap, self.slots
        st[LEVEL:LEVEL + 1] += 1
        env.action_mask(self.front_ids, out=self.mask)
        flags = ((self.mask[:, :1] >> self.six) & 1) * (self.front_ids < st[FRONT]).to(torch.uint8).unsqueeze(1)
        self.pairs = sel.select(keep=flags, k=slots, out=self.pairs)                      # a fixed-shape nonzero
        if self.check:
            self._check_pairs(flags)
        pair = self.pairs.index
        valid = pair >= 0
        parent = torch.where(valid, pair // (ACTIONS - 1), 0)
        action = torch.where(valid, pair % (ACTIONS - 1), DONE)
        self.snap_children = env.snapshot(parent, out=self.snap_children)                 # the fork, through buffers kept
        env.restore(self.snap_children, self.child_ids)
        self.act[cap:cap + slots, 0] = action.to(torch.int8)
        env.step(self.act)
        found = ((env.agents[cap:cap + slots, 0, 4] != 0) & valid).any()
        env.state_key(self.child_ids, out=self.keys)
        self.res = self.table.insert(self.keys, count=False, out=self.res)
        env.agent_distance(self.child_ids, types=[Type.goal], out=self.dist)
        fresh = self.res.is_new & valid
        entry = torch.where(fresh, self.res.entry, self.table.capacity)
        self.depth_of.scatter_(0, entry, st[LEVEL:LEVEL + 1].expand(slots))
        d = self.dist[:, 0].to(torch.int64)
        score = (self.depth_of[entry] + torch.where(d < 0, FAR, d)).to(torch.int32)
        self.nxt = sel.select(score, fresh, k=self.beam, values=self.child_ids, fill=0, out=self.nxt)      # the beam cut
        if self.check:
            self._check_beam(score, fresh)
        self.snap_front = env.snapshot(self.nxt.index, out=self.snap_front)
        env.restore(self.snap_front, self.front_ids[:self.beam])
        st[FRONT:FRONT + 1] = self.nxt.count[:1]
        st[FOUND:FOUND + 1] = torch.maximum(st[FOUND:FOUND + 1], found.to(torch.int64))
        st[CHILDREN:CHILDREN + 1] = self.nxt.count[1:]

    # ---- --check: both selections against torch, from the same tensors (eager only: it reads the counts) ---------------------------
    def _check_pairs(self, flags):
        want = torch.nonzero(flags.reshape(-1)).squeeze(1)
        m, total = self.pairs.count.tolist()
        assert m == total == want.numel() <= self.slots, (m, total, want.numel())
        assert torch.equal(self.pairs.index[:m], want) and bool((self.pairs.index[m:] == -1).all())
        self.checked += 1

    def _check_beam(self, score, keep):
        m, total = self.nxt.count.tolist()
        assert total == int(keep.sum()) and m == min(self.beam, total), (m, total)
        order = torch.argsort(torch.where(keep, score.to(torch.int64), BIG), stable=True)[:m]
        assert torch.equal(self.nxt.index[:m], self.child_ids[order.sort().values]) and bool((self.nxt.index[m:] == 0).all())
        self.checked += 1


def search(env, table, roots, beam, depth, check=False, graph=False):
    """level by level from the envs [0, roots); the host reads the status tensor once per level"""
    lv = Level(env, table, beam, check)
    lv.root(roots)
    step = lv.run
    if graph:
        # warm up on a side stream (every buffer a level keeps is allocated there), put the state back, then capture
        dev = env.agents.device
        saved = (env.snapshot(), table.state_dict(), lv.status.clone(), lv.depth_of.clone())
        cur, side, g = torch.cuda.current_stream(dev), torch.cuda.Stream(dev), torch.cuda.CUDAGraph()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            lv.run()
            env.restore(saved[0])
            table.load_state_dict(saved[1])
            lv.status.copy_(saved[2])
            lv.depth_of.copy_(saved[3])
            with torch.cuda.graph(g, stream=side):
                lv.run()
        cur.wait_stream(side)
        step = g.replay
    history, expanded, front = [], 0, min(roots, lv.cap)
    for _ in range(depth):
        expanded += front
        step()
        history.append(lv.status.tolist())                                     # the level's one read
        front = history[-1][FRONT]
        if history[-1][FOUND] or front == 0:
            break
    return {"nodes_expanded": expanded, "depth": history[-1][LEVEL] if history else 0, "found": bool(history and history[-1][FOUND]),
            "new_per_level": [h[CHILDREN] for h in history], "history": history, "selections_checked": lv.checked}


def run(workload="c2", roots=1, beam=8, depth=40, batch=None, device="cuda:0", backend=None, capacity=1 << 14, check=False,
        graph=False):
    if check and graph:
        raise ValueError("graph_search: --check reads the counts at every level and runs eagerly; not with --graph")
    dev = torch.device(device)
    wl = workloads.make(workload, batch=batch)
    if not (wl.grid[..., 0] == int(Type.goal)).any():
        raise ValueError(f"graph_search: workload {workload} has no goal cell for the heuristic to aim at")
    env = wl.make_env(dev, auto_reset=False, **({"backend": backend} if backend is not None else {}))
    table = env.key_table(capacity)
    out = {"workload": wl.title, "batch": wl.batch, "roots": roots, "beam": beam, "capacity": capacity, "checked": bool(check),
           "graph": bool(graph)}
    out.update(search(env, table, roots, beam, depth, check, graph))
    out["table_entries"], out["drops"] = table.entries(), table.dropped()
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
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args()
    print(json.dumps(run(a.workload, a.roots, a.beam, a.depth, capacity=a.capacity, check=a.check, graph=a.graph)))
