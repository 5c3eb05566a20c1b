#!/usr/bin/env python3
"""What a restore of n chosen envs (BatchedMultiGridEnv.restore -> mgx_env_copy, csrc/mgx_env_copy.hip) costs.  GPU box.

The kernel alone, on state sets of the benchmark's shapes with the members a pool-restarted env carries (cells, agents, rng,
step_count, aux, marker, episode): a snapshot of n rows restored into n random DISTINCT envs of the batch.

    C4  Empty-16x16, 4 agents, 16-bit cells (512-byte tiles), 65 536 envs:  n = 64, 4 096, 65 536
    C5  64x64, 16 agents, compact cells (4 096-byte tiles), 32 768 envs:    n = 32 768

Each point against two references measured in the same run, alternating with it:
    torch   the torch formulation of the same copy: index_select + index_copy_ per member over the same tensors (14 launches)
    copy_   a plain copy_ of the same number of bytes between two flat buffers: the streaming bound

Every candidate is captured as a graph of REPS back-to-back calls and timed with device events over a replay (per call = / REPS);
PASSES replays after WARM warm ones: the median and the spread (min, max).  The result of the kernel is compared with the torch
formulation's bit for bit before anything is timed.  No time is asserted.

Usage: python tools/env_snapshot_bench.py [--out profiles/env_snapshot.txt]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigrid_amd import EnvSpec, _lib  # noqa: E402
from multigrid_amd.ops import HipBackend  # noqa: E402

REPS, PASSES, WARM = 20, 15, 3
DEV = torch.device("cuda:0")
POINTS = (("C4 Empty-16x16 A=4 16-bit cells", EnvSpec(16, 16, 4, 7), 65536, (64, 4096, 65536)),
          ("C5 64x64 A=16 compact cells", EnvSpec(64, 64, 16, 9, cell_bytes=1), 32768, (32768,)))


def state_set(spec, rows, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    rnd = lambda shape, dt, hi=127: torch.randint(0, hi, shape, dtype=dt, device=DEV, generator=g)
    return {"cells": rnd(tuple(spec.cells_shape(rows)), torch.int16 if spec.cell_bytes == 2 else torch.uint8),
            "agents": rnd(tuple(spec.agents_shape(rows)), torch.uint8), "rng": rnd((rows, 4), torch.int64, 2 ** 40),
            "step_count": rnd((rows,), torch.int32), "aux": rnd((rows, 16), torch.uint8), "marker": rnd((rows,), torch.int32),
            "episode": rnd((rows,), torch.int32)}


def graph_of(fn):
    stream = torch.cuda.current_stream(DEV)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(DEV)
    side.wait_stream(stream)
    with torch.cuda.stream(side):
        fn()                                                    # (warm: code objects loaded, the allocator's blocks made)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(REPS):
                fn()
    stream.wait_stream(side)
    return graph


def measure(graphs):
    """{name: [microseconds per call of every pass]}: the candidates alternate inside a pass"""
    out = {k: [] for k in graphs}
    for p in range(WARM + PASSES):
        for k, gr in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            if p >= WARM:
                out[k].append(a.elapsed_time(b) * 1000.0 / REPS)
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"tools/env_snapshot_bench.py on {torch.cuda.get_device_name(0)}: a restore of n rows into n random distinct envs; microseconds",
             f"per call, median (min, max) of {PASSES} graph replays of {REPS} calls each after {WARM} warm ones; GB/s = bytes read + written",
             "over the median.  kernel = mgx_env_copy (one launch); torch = index_select + index_copy_ per member (14 launches); copy_ =",
             "one plain copy_ of the same bytes.", ""]
    for title, spec, B, ns in POINTS:
        be = HipBackend(spec, DEV)
        env, ref = state_set(spec, B, 1), None
        row_bytes = sum(t[0].numel() * t.element_size() for t in env.values())
        lines.append(f"{title}, {B} envs, {row_bytes} bytes per env")
        for n in ns:
            snap = state_set(spec, n, 2)
            ids = torch.randperm(B, device=DEV)[:n].contiguous()
            rows = torch.arange(n, device=DEV)
            bad = torch.tensor([0, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
            flat_a = torch.zeros(n * row_bytes, dtype=torch.uint8, device=DEV)
            flat_b = torch.ones(n * row_bytes, dtype=torch.uint8, device=DEV)

            def kernel():
                be.env_copy(n, snap, n, None, env, B, ids, None, _lib.STAGE_NONE, False, bad)

            def chain(dst=None):
                for m, t in (env if dst is None else dst).items():
                    t.index_copy_(0, ids, snap[m].index_select(0, rows))

            # the same result, bit for bit
            ref = {m: t.clone() for m, t in env.items()}
            chain(ref)
            kernel()
            torch.cuda.synchronize()
            assert bad.tolist() == [0, 2 ** 31 - 1]
            for m in env:
                assert torch.equal(env[m], ref[m]), m
            res = measure({"kernel": graph_of(kernel), "torch": graph_of(chain), "copy_": graph_of(lambda: flat_a.copy_(flat_b))})
            moved = 2 * n * row_bytes
            cells = []
            for k in ("kernel", "torch", "copy_"):
                v = sorted(res[k])
                med = v[len(v) // 2]
                cells.append(f"{k} {med:9.2f} ({v[0]:.2f}, {v[-1]:.2f}) {moved / med / 1e3:7.1f} GB/s")
            kmed, tmed, cmed = (sorted(res[k])[PASSES // 2] for k in ("kernel", "torch", "copy_"))
            lines.append(f"  n = {n:6d}  " + "   ".join(cells) + f"   torch / kernel {tmed / kmed:5.2f}   kernel / copy_ {kmed / cmed:5.2f}")
            del snap, flat_a, flat_b, ref
        lines.append("")
        del env
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
