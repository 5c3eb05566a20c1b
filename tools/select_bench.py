#!/usr/bin/env python3
"""What the device selection costs (multigrid_amd.Selector -> mgx_select, csrc/mgx_select.hip), against the fixed-shape torch
formulation `argsort(where(keep, score, BIG), stable=True)[:k]` on the same tensors, in the same process, on the same GPU.  GPU box.

The sizes are those of a search level at BASELINE.json's C2, C4 and C5 shapes (4 096, 65 536 and 32 768 envs): n = 6 * (B // 7) child
slots.  Two calls are timed per size:
    the beam cut     select(score, keep, k=4096) (C2: k=512): six launches
    the compaction   select(keep=keep, k=n): two launches -- a `nonzero` of fixed shape; torch's side is the same argsort with every
                     score equal
with the scores distinct (a permutation), in 0..63 (a level's real spread: depth + distance) and all equal, and keep at 1 %, 50 % and
100 %.

The launches are timed as graph replays of REPS calls between two events, median (min, max) of PASSES replays after WARM warm ones,
the two candidates alternating inside a pass.  In cache: the replays follow each other, the inputs (at most 0.7 MB) stay in the L2s;
nothing is flushed.  Every result is checked against torch's (sorted, cut at the count) before anything is timed.  No time is asserted.

Usage: python tools/select_bench.py [--out FILE]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multigrid_amd import Selector  # noqa: E402

REPS, PASSES, WARM = 20, 15, 3
DEV = torch.device("cuda:0")
POINTS = (("C2", 4096, 512), ("C4", 65536, 4096), ("C5", 32768, 4096))
BIG = 1 << 40


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


def fmt(v):
    return f"{v[len(v) // 2]:8.2f} ({v[0]:.2f}, {v[-1]:.2f})"


def torch_select(score, keep, k):
    return torch.argsort(torch.where(keep, score, BIG), stable=True)[:k]


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"tools/select_bench.py on {torch.cuda.get_device_name(0)}: microseconds per call, median (min, max) of {PASSES} graph replays of {REPS}",
             f"calls each after {WARM} warm ones, the two candidates alternating.  select = Selector.select (six launches with scores, two",
             "without); torch = argsort(where(keep, score, BIG), stable=True)[:k] in the same kind of graph.  In cache, nothing flushed.", ""]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    for title, B, beam in POINTS:
        n = 6 * (B // 7)
        sel = Selector(n, DEV)
        lines.append(f"{title}: B = {B}, n = {n} child slots, beam cut k = {beam}, compaction k = n; {-(-n // 256)} workgroups a launch")
        scores = {"distinct": torch.randperm(n, device=DEV, generator=gen).to(torch.int32),
                  "0..63": torch.randint(0, 64, (n,), device=DEV, generator=gen, dtype=torch.int32),
                  "equal": torch.full((n,), 17, dtype=torch.int32, device=DEV), None: None}
        for kind, score in scores.items():
            for share in (0.01, 0.5, 1.0):
                keep = torch.rand(n, device=DEV, generator=gen) < share
                k = beam if score is not None else n
                wide = score.to(torch.int64) if score is not None else torch.zeros(n, dtype=torch.int64, device=DEV)
                res = sel.select(score, keep, k=k)
                m, total = res.count.tolist()
                want = torch_select(wide, keep, k)[:m].sort().values
                assert total == int(keep.sum()) and m == min(k, total) and torch.equal(res.index[:m], want) and bool((res.index[m:] == -1).all())
                got = measure({"select": graph_of(lambda: sel.select(score, keep, k=k, out=res), REPS),
                               "torch": graph_of(lambda: torch_select(wide, keep, k), REPS)})
                ours, theirs = got["select"][len(got["select"]) // 2], got["torch"][len(got["torch"]) // 2]
                what = f"beam cut, scores {kind}" if score is not None else "compaction, no scores"
                lines.append(f"  {what:26s} keep {int(share * 100):3d} %: select {fmt(got['select'])}   torch {fmt(got['torch'])}   "
                             f"torch / select {theirs / ours:5.1f}{'   SLOWER THAN TORCH' if ours > theirs else ''}")
        lines.append("")
        del sel
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
