#!/usr/bin/env python3
"""What the walking-distance fields of a whole batch cost (BatchedMultiGridEnv.distance_field / agent_distance -> mgx_distance,
csrc/mgx_distance.hip), against the launches that read the same state once and against the torch-op formulation of the same rule.
GPU box.

At BASELINE.json's C2, C4 and C5 shapes, for all B envs of the workload's first layout with the agents on random interior cells:

    agent_dist  agent_distance(types=[goal]): i16[B, A]
    field       distance_field(types=[goal]): i16[B, H, W]
    snapshot    agent_distance(types=[goal]) of a snapshot's rows
    key, mask   state_key() and action_mask() of the same envs: the launches that read the same state once
    torch       the same rule in torch ops, written here: boolean dilation over `env.grid`, iterated to the fixed point -- what a user
                does without the kernel.  Eager calls between two events (its trip count depends on the data: a host round trip per
                level), three passes.

The kernel launches are timed as graph replays of REPS calls between two events, median (min, max) of PASSES replays after WARM warm
ones, the candidates alternating inside a pass.  The fraction of the byte roofline counts the tile read once and 2 bytes written per
cell (or per agent) against PEAK_BYTES_PER_S.  The field and the agents' distances of the first 256 envs are checked against the
NumPy rule (tests/test_distance.py) before anything is timed.  The 2078-level serpentine (a correctness case of
tests/test_distance_gpu.py) is timed once, as the worst case.  No time is asserted.

Usage: python tools/distance_bench.py [--out profiles/distance.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multigrid_amd import BatchedMultiGridEnv, workloads  # noqa: E402
from multigrid_amd.constants import Type  # noqa: E402

REPS, PASSES, WARM, TORCH_PASSES = 20, 15, 3, 3
PEAK_BYTES_PER_S = 8.0e12                                        # MI355X HBM3E, the data-sheet figure
DEV = torch.device("cuda:0")
POINTS = (("C2 Empty-16x16 A=4 16-bit cells", "c2", 4096), ("C4 Empty-16x16 A=4 16-bit cells", "c4", 65536),
          ("C5 64x64 A=16 compact cells", "c5", 32768))
GOAL = [Type.goal]


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
    return out


def torch_field(env):
    """the rule of include/mgx.h "DISTANCE FIELDS" for types=[goal], no flags, in torch ops over env.grid -> (i16[B,H,W], levels)"""
    g = env.grid
    t, s = g[..., 0] & 15, g[..., 2] & 3
    passable = (t == 1) | (t == 3) | (t == 8) | (t == 9) | ((t == 4) & (s == 0))
    front = t == 8
    seen = front.clone()
    d = torch.full(t.shape, -1, dtype=torch.int16, device=g.device)
    d[front] = 0
    level = 0
    while bool(front.any()):
        level += 1
        nb = torch.zeros_like(front)
        nb[:, 1:] |= front[:, :-1]
        nb[:, :-1] |= front[:, 1:]
        nb[:, :, 1:] |= front[:, :, :-1]
        nb[:, :, :-1] |= front[:, :, 1:]
        front = nb & passable & ~seen
        d[front] = level
        seen |= front
    return d, level - 1


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


def check_against_the_model(env, field, dist, n=256):
    from tests.test_distance import model_distance
    want_f, want_a = model_distance(3, env.grid[:n].cpu().numpy(), env.agents[:n].cpu().numpy(), env.spec, type_mask=1 << int(Type.goal))
    assert field[:n].cpu().numpy().tolist() == want_f.tolist(), "the kernel's field differs from the model's"
    assert dist[:n].cpu().numpy().tolist() == want_a.tolist(), "the kernel's agent distances differ from the model's"


def serpentine_line():
    from tests.test_distance_gpu import serpentine
    wl = workloads.make("c5", batch=1, global_batch=1024)
    snake, end, far = serpentine(64, 64)
    env = BatchedMultiGridEnv(wl.spec, 1024, DEV)
    env.load_state(snake, wl.agents[0], validate=False)
    pts = torch.zeros((1024, 1, 2), dtype=torch.int16, device=DEV)
    field = torch.zeros((1024, 64, 64), dtype=torch.int16, device=DEV)
    env.distance_field(points=pts, out=field)
    torch.cuda.synchronize()
    assert int(field[0, end[1], end[0]]) == far == 2078 and int(field.max()) == far
    v = time_eager(lambda: env.distance_field(points=pts, out=field), 5)
    return (f"worst case: the 64x64 serpentine, {far} levels, 1024 envs (one wavefront each), one launch between two events: "
            f"{v[len(v) // 2]:.1f} us ({v[0]:.1f}, {v[-1]:.1f})")


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"tools/distance_bench.py on {torch.cuda.get_device_name(0)}: walking distances to the goal cells for all B envs; microseconds per call,",
             f"median (min, max) of {PASSES} graph replays of {REPS} calls each after {WARM} warm ones.  agent_dist = agent_distance(types=[goal]),",
             "i16[B, A]; field = distance_field(types=[goal]), i16[B, H, W]; snapshot = agent_dist over a snapshot's rows; key / mask =",
             "mgx_state_key / mgx_action_mask of the same envs, the launches that read the same state once; torch = the same rule as boolean",
             f"dilation over env.grid iterated to the fixed point, eager, {TORCH_PASSES} passes.  roofline = (tile bytes + 2 bytes per output value) /",
             f"time against {PEAK_BYTES_PER_S / 1e12:.1f} TB/s.  levels = the deepest level of the batch.  The agents stand on random interior cells.", ""]
    for title, name, B in POINTS:
        wl = workloads.make(name, batch=1, global_batch=B)
        spec, A = wl.spec, wl.spec.num_agents
        env = BatchedMultiGridEnv(spec, B, DEV)
        env.load_state(wl.grid[0], wl.agents[0], validate=False)
        g = torch.Generator(device=DEV); g.manual_seed(1)
        env.agents[:, :, 2] = torch.randint(1, spec.width - 1, (B, A), dtype=torch.uint8, device=DEV, generator=g)
        env.agents[:, :, 3] = torch.randint(1, spec.height - 1, (B, A), dtype=torch.uint8, device=DEV, generator=g)
        H, W = spec.height, spec.width
        dist = torch.zeros((B, A), dtype=torch.int16, device=DEV)
        field = torch.zeros((B, H, W), dtype=torch.int16, device=DEV)
        mask = torch.zeros((B, A), dtype=torch.uint8, device=DEV)
        keys = torch.zeros(B, dtype=torch.int64, device=DEV)
        snap = env.snapshot()
        env.agent_distance(types=GOAL, out=dist)
        env.distance_field(types=GOAL, out=field)
        torch.cuda.synchronize()
        check_against_the_model(env, field, dist)
        ref, levels = torch_field(env)
        assert torch.equal(ref, field), "the torch formulation and the kernel disagree"
        env.check_errors()
        res = measure({"agent_dist": graph_of(lambda: env.agent_distance(types=GOAL, out=dist), REPS),
                       "field": graph_of(lambda: env.distance_field(types=GOAL, out=field), REPS),
                       "snapshot": graph_of(lambda: snap.agent_distance(types=GOAL, out=dist), REPS),
                       "key": graph_of(lambda: env.state_key(out=keys), REPS),
                       "mask": graph_of(lambda: env.action_mask(out=mask), REPS)})
        tor = time_eager(lambda: torch_field(env), TORCH_PASSES)
        tile = env._cells[0].numel() * env._cells.element_size()
        moved = {"agent_dist": B * (tile + 2 * A), "field": B * (tile + 2 * H * W), "snapshot": B * (tile + 2 * A)}
        lines.append(f"{title}, {B} envs, {tile}-byte tiles, {levels} levels, {int((field >= 0).sum()) // B} reachable cells per env")
        med = {}
        for k in ("agent_dist", "field", "snapshot", "key", "mask"):
            v = sorted(res[k])
            med[k] = v[len(v) // 2]
            roof = f"   roofline {moved[k] / (med[k] * 1e-6) / PEAK_BYTES_PER_S:6.1%}" if k in moved else ""
            lines.append(f"  {k:11s}{med[k]:10.2f} ({v[0]:.2f}, {v[-1]:.2f}){roof}")
        lines.append(f"  {'torch':11s}{tor[len(tor) // 2]:10.1f} ({tor[0]:.1f}, {tor[-1]:.1f})")
        lines.append(f"  agent_dist / key {med['agent_dist'] / med['key']:5.2f}   field / key {med['field'] / med['key']:5.2f}   "
                     f"torch / field {tor[len(tor) // 2] / med['field']:7.1f}")
        lines.append("")
        del env, snap, dist, field, mask, keys, ref
        torch.cuda.empty_cache()
    lines.append(serpentine_line())
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
