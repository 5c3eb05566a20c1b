#!/usr/bin/env python3
"""What the device key tables cost (multigrid_amd.KeyTable -> mgx_key_insert / mgx_key_lookup, csrc/mgx_key_table.hip), against the
torch formulation of examples/best_first.py on the same keys, in the same process, on the same GPU.  GPU box.

The keys.  At BASELINE.json's C2, C4 and C5 shapes (4 096, 65 536 and 32 768 envs) the frontier of examples/masked_expand.py is grown
from 8 roots -- mask, fork, step, key, keep one env per distinct state -- for LEVELS levels or until the batch is full, and the keys
are `state_key()` of all B envs after the last level: forked and stepped envs, with the duplicates such an expansion leaves.  The
share of duplicates (1 - distinct / B) is printed.

What is timed, per point, with a table of CAPACITY slots pre-filled with random keys to a load of 0.1 and of 0.5:
    insert      table.insert(keys, first=True, visits=True, out=...): both launches.  After the warm call the level's keys are in the
                table, so this is the steady state of a search that meets mostly known states.
    lookup      table.lookup(keys, visits=True, out=...): one launch
    torch       uniq, inverse = unique(keys, return_inverse=True); scatter_reduce_(amin); isin(uniq, seen); cat((seen, new)) -- with
                `seen` holding as many keys as the table does.  Eager between two events (unique's output size is a host round trip).
and the two worst cases, B keys into the table at load 0.1:
    one key     every key equal: all indices meet in ONE slot's two words (an atomic max on the tag, an atomic add on the count).
                The kernel merges equal keys inside a wavefront before they go to memory, so the slot takes one pair of atomics per
                wavefront, B / 64 a call; printed beside the time are the indices per microsecond and those atomics per microsecond
                on one word, whose yardstick is the ~88 per microsecond at which one word saturates under returning atomic adds
                (these two do not return a value).  The same case WITHOUT the merge is a build of its own (the kernel before the
                merge was added); its figures are kept at the end of profiles/key_table.txt.
    all new     B random keys nobody has seen: the table is put back (one copy of its buffer) before every insert; the copy alone is
                timed too and both figures are given.

The launches are timed as graph replays of REPS calls between two events, median (min, max) of PASSES replays after WARM warm ones,
the candidates alternating inside a pass.  In cache: the replays follow each other, so the table (24 bytes a slot: 6 MiB at 2^18) and
the keys stay in the L2s / the Infinity Cache between calls; nothing is flushed.  The outputs are checked against the torch
formulation before anything is timed.  No time is asserted.

Usage: python tools/key_table_bench.py [--out profiles/key_table.txt]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multigrid_amd import KeyTable, workloads  # noqa: E402

REPS, PASSES, WARM, TORCH_PASSES, LEVELS = 20, 15, 3, 7, 12
CAPACITY = 1 << 18
DEV = torch.device("cuda:0")
POINTS = (("C2 Empty-16x16 A=4", "c2", 4096), ("C4 Empty-16x16 A=4", "c4", 65536), ("C5 64x64 A=16 compact cells", "c5", 32768))
DONE, ACTIONS = 6, 7
ONE_WORD_RATE = 88.0                                              # returning atomic adds per microsecond at which one word saturates


def graph_of(fn, reps):
    stream = torch.cuda.current_stream(DEV)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(DEV)
    side.wait_stream(stream)
    with torch.cuda.stream(side):
        fn()                                                    # (warm: code objects loaded, the allocator's blocks made)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(reps):
                fn()
    stream.wait_stream(side)
    return graph, reps


def measure(graphs):
    """{name: [microseconds per call of every pass]}: the candidates alternate inside a pass"""
    out = {k: [] for k in graphs}
    for p in range(WARM + PASSES):
        for k, (gr, reps) in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            if p >= WARM:
                out[k].append(a.elapsed_time(b) * 1000.0 / reps)
    return {k: sorted(v) for k, v in out.items()}


def time_eager(fn, passes):
    out = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0)
    return sorted(out)


def fmt(v):
    return f"{v[len(v) // 2]:9.2f} ({v[0]:.2f}, {v[-1]:.2f})"


def level_keys(name, B):
    """the keys of all B envs after growing masked_expand's frontier from 8 roots -> (int64 [B], levels run, the last frontier)"""
    wl = workloads.make(name)
    assert wl.batch == B, (name, wl.batch)
    env = wl.make_env(DEV, auto_reset=False)
    cap, six = B // ACTIONS, torch.arange(ACTIONS - 1, device=DEV)
    F, levels = 8, 0
    for levels in range(1, LEVELS + 1):
        ids = torch.arange(F, device=DEV)
        mask = env.action_mask(ids)
        parent, action = torch.nonzero((mask[:, :1] >> six) & 1, as_tuple=True)
        n = int(parent.numel())
        dst = torch.arange(F, F + n, device=DEV)
        if n:
            env.fork(parent.contiguous(), dst)
        act = torch.full((B, env.spec.num_agents), DONE, dtype=torch.int8, device=DEV)
        act[dst, 0] = action.to(torch.int8)
        env.step(act)
        keys = env.state_key(torch.arange(F + n, device=DEV))
        uniq, inverse = torch.unique(keys, return_inverse=True)
        first = torch.full((uniq.numel(),), B, dtype=torch.int64, device=DEV).scatter_reduce_(
            0, inverse, torch.arange(keys.numel(), device=DEV), reduce="amin")[:cap]
        full = int(first.numel()) == cap
        F = int(first.numel())
        env.fork(first.contiguous(), torch.arange(F, device=DEV))
        if full:
            break
    keys = env.state_key().clone()
    env.check_errors()
    return keys, levels, F


def torch_level(keys, seen):
    n = keys.numel()
    uniq, inverse = torch.unique(keys, return_inverse=True)
    first = torch.full((uniq.numel(),), n, dtype=torch.int64, device=DEV).scatter_reduce_(0, inverse, torch.arange(n, device=DEV), reduce="amin")
    fresh = ~torch.isin(uniq, seen)
    return first[fresh], first[inverse], torch.cat((seen, uniq[fresh]))


def filled(load, gen):
    """a table of CAPACITY slots holding load * CAPACITY random keys, and those keys"""
    t = KeyTable(CAPACITY, DEV)
    seen = torch.randint(-(1 << 62), 1 << 62, (int(load * CAPACITY),), dtype=torch.int64, device=DEV, generator=gen)
    t.insert(seen, is_new=False)
    assert t.dropped() == 0
    return t, seen


def outputs(n):
    z = lambda dt: torch.zeros(n, dtype=dt, device=DEV)
    return z(torch.int64), z(torch.bool), z(torch.int64), z(torch.int32)


def main():
    from multigrid_amd import KeyInsert, KeyLookup
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"tools/key_table_bench.py on {torch.cuda.get_device_name(0)}: microseconds per call, median (min, max) of {PASSES} graph replays of {REPS}",
             f"calls each after {WARM} warm ones; torch = unique + scatter_reduce(amin) + isin + cat, eager between two events, {TORCH_PASSES} passes, with",
             f"`seen` as large as the table's contents.  Tables of 2^{CAPACITY.bit_length() - 1} slots ({24 * CAPACITY // 2 ** 20} MiB) pre-filled with random keys to the load given.",
             "insert = both launches, first / visits / is_new / entry written; the level's keys are in the table after the warm call (a search",
             "that meets known states).  In cache: replays follow each other, the table and the keys stay in L2 / Infinity Cache; no flush.", ""]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    for title, name, B in POINTS:
        keys, levels, F = level_keys(name, B)
        distinct = int(torch.unique(keys).numel())
        lines.append(f"{title}: {B} keys of state_key() after {levels} levels of examples/masked_expand.py's expansion from 8 roots (last frontier {F}): "
                     f"{distinct} distinct, duplicate share {1 - distinct / B:.3f}")
        for load in (0.1, 0.5):
            t, seen = filled(load, gen)
            res, found = KeyInsert(*outputs(B)), KeyLookup(*outputs(B)[::3])
            t.insert(keys, first=True, visits=True, out=res)
            want_new, want_first, seen_after = torch_level(keys, seen)
            assert torch.nonzero(res.is_new).squeeze(1).tolist() == sorted(want_new.tolist()) and torch.equal(res.first, want_first)
            assert torch.equal(t.lookup(keys, visits=True, out=found).entry, res.entry) and t.dropped() == 0
            got = measure({"insert": graph_of(lambda: t.insert(keys, first=True, visits=True, out=res), REPS),
                           "lookup": graph_of(lambda: t.lookup(keys, visits=True, out=found), REPS)})
            tor = time_eager(lambda: torch_level(keys, seen_after), TORCH_PASSES)
            lines.append(f"  load {load}: {t.entries()} entries   insert {fmt(got['insert'])}   lookup {fmt(got['lookup'])}   "
                         f"torch {fmt(tor)} with {seen_after.numel()} seen   torch / insert {tor[len(tor) // 2] / got['insert'][len(got['insert']) // 2]:.1f}")
            del t, seen, seen_after
        # the worst cases, at load 0.1
        t, seen = filled(0.1, gen)
        before = t._buf.clone()
        res = KeyInsert(*outputs(B))
        same = torch.full((B,), 0x1234567, dtype=torch.int64, device=DEV)
        fresh = torch.randint(-(1 << 62), 1 << 62, (B,), dtype=torch.int64, device=DEV, generator=gen)

        def put_back_and_insert():
            t._buf.copy_(before)
            t.insert(fresh, first=True, visits=True, out=res)
        got = measure({"one": graph_of(lambda: t.insert(same, first=True, visits=True, out=res), REPS),
                       "new": graph_of(put_back_and_insert, REPS), "copy": graph_of(lambda: t._buf.copy_(before), REPS)})
        assert int(res.is_new.sum()) == int(torch.unique(fresh).numel()) and t.dropped() == 0
        tor_one = time_eager(lambda: torch_level(same, seen), TORCH_PASSES)
        tor_new = time_eager(lambda: torch_level(fresh, seen), TORCH_PASSES)
        one = got["one"][len(got["one"]) // 2]
        new, copy = got["new"][len(got["new"]) // 2], got["copy"][len(got["copy"]) // 2]
        lines.append(f"  worst, every key equal: insert {fmt(got['one'])} = {B / one:.0f} indices per us; merged per wavefront, each of the slot's two "
                     f"words takes {B // 64} atomics a call, {B / 64 / one:.1f} per us (yardstick: one word saturates near {ONE_WORD_RATE:.0f} "
                     f"returning adds per us)   torch {fmt(tor_one)}")
        lines.append(f"  worst, every key new:   put back + insert {fmt(got['new'])}, the put-back copy alone {fmt(got['copy'])}: insert about "
                     f"{new - copy:.2f}   torch {fmt(tor_new)}")
        lines.append("")
        del t, seen, before
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
