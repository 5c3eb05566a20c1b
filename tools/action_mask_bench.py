#!/usr/bin/env python3
"""What the effective-action masks of a whole batch cost (BatchedMultiGridEnv.action_mask -> mgx_action_mask,
csrc/mgx_action_mask.hip), against the state keys of the same envs.  GPU box.

The kernel alone, on live envs of the benchmark's shapes, masks of all B envs:

    C2  Empty-16x16, 4 agents, 16-bit cells (512-byte tiles),   4 096 envs
    C4  the same shape,                                         65 536 envs
    C5  64x64, 16 agents, compact cells (4 096-byte tiles),    32 768 envs

Every env holds the configuration's first start with its agents moved to random interior cells and turned at random, so that the
front cells -- the one gather an agent makes -- are spread over the tile as they are in a running batch (the kernel has no other
data-dependent path).  Three candidates, measured in the same run, alternating:

    mask      mgx_action_mask, u8[B, A]
    expanded  mgx_action_mask with MGX_MASK_EXPAND, bool[B, A, 7]
    key       mgx_state_key of the same envs (no flags): unchanged by the masks, the yardstick -- it reads the whole tile where
              a mask reads the agent rows and one sector per agent

Every candidate is captured as a graph of REPS back-to-back calls and timed with device events over a replay (per call = / REPS);
PASSES replays after WARM warm ones: the median and the spread (min, max).  The masks of the first 256 envs are compared with the
NumPy statement of the rule (tests/test_action_mask.py) before anything is timed.  No time is asserted.

Usage: python tools/action_mask_bench.py [--out profiles/action_mask.txt]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multigrid_amd import BatchedMultiGridEnv, workloads  # noqa: E402

REPS, PASSES, WARM = 20, 15, 3
DEV = torch.device("cuda:0")
POINTS = (("C2 Empty-16x16 A=4 16-bit cells", "c2", 4096), ("C4 Empty-16x16 A=4 16-bit cells", "c4", 65536),
          ("C5 64x64 A=16 compact cells", "c5", 32768))


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


def check_against_the_model(env, mask, wide, n=256):
    from tests.test_action_mask import expanded, model_action_mask
    want = model_action_mask(3, env.grid[:n].cpu().numpy(), env.agents[:n].cpu().numpy(), env.aux[:n].cpu().numpy(), env.spec)
    assert mask[:n].cpu().numpy().tolist() == want.tolist(), "the kernel's masks differ from the model's"
    assert wide[:n].cpu().numpy().tolist() == expanded(want).astype(bool).tolist(), "the expanded masks differ from the model's"


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"tools/action_mask_bench.py on {torch.cuda.get_device_name(0)}: the effective-action masks of all B envs; microseconds per call,",
             f"median (min, max) of {PASSES} graph replays of {REPS} calls each after {WARM} warm ones.  mask = mgx_action_mask, u8[B, A];",
             "expanded = the same launch with MGX_MASK_EXPAND, bool[B, A, 7]; key = mgx_state_key of the same envs (no flags), the",
             "yardstick: it reads every env's whole tile, a mask its agent rows and one front cell per agent.  The agents stand on random",
             "interior cells, turned at random.  The masks of the first 256 envs are checked against the NumPy rule first.", ""]
    for title, name, B in POINTS:
        wl = workloads.make(name, batch=1, global_batch=B)
        spec, A = wl.spec, wl.spec.num_agents
        env = BatchedMultiGridEnv(spec, B, DEV)
        env.load_state(wl.grid[0], wl.agents[0], validate=False)
        g = torch.Generator(device=DEV); g.manual_seed(1)
        env.agents[:, :, 1] = torch.randint(0, 4, (B, A), dtype=torch.uint8, device=DEV, generator=g)
        env.agents[:, :, 2] = torch.randint(1, spec.width - 1, (B, A), dtype=torch.uint8, device=DEV, generator=g)
        env.agents[:, :, 3] = torch.randint(1, spec.height - 1, (B, A), dtype=torch.uint8, device=DEV, generator=g)
        mask = torch.zeros((B, A), dtype=torch.uint8, device=DEV)
        wide = torch.zeros((B, A, 7), dtype=torch.bool, device=DEV)
        keys = torch.zeros(B, dtype=torch.int64, device=DEV)
        env.action_mask(out=mask)
        env.action_mask(expand=True, out=wide)
        torch.cuda.synchronize()
        check_against_the_model(env, mask, wide)
        env.check_errors()
        res = measure({"mask": graph_of(lambda: env.action_mask(out=mask), REPS),
                       "expanded": graph_of(lambda: env.action_mask(expand=True, out=wide), REPS),
                       "key": graph_of(lambda: env.state_key(out=keys), REPS)})
        med = {}
        tile = env._cells[0].numel() * env._cells.element_size()
        lines.append(f"{title}, {B} envs, {tile}-byte tiles, {B * A} agents, {len(torch.unique(mask))} distinct masks")
        for k in ("mask", "expanded", "key"):
            v = sorted(res[k])
            med[k] = v[len(v) // 2]
            lines.append(f"  {k:9s}{med[k]:9.2f} ({v[0]:.2f}, {v[-1]:.2f})")
        lines.append(f"  mask / key {med['mask'] / med['key']:5.2f}   expanded / key {med['expanded'] / med['key']:5.2f}")
        lines.append("")
        del env, mask, wide, keys
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
