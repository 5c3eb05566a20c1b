#!/usr/bin/env python3
"""Frame rendering throughput (BatchedMultiGridEnv.render -> include/mgx.h mgx_render) on the MI355X.

    python tools/render_bench.py [--iters N] [--out profiles/render_bench.txt]
    rocprofv3 --kernel-trace --stats -d render_prof -o r -- python tools/render_bench.py --iters 20   (kernel times)

Cases: 1 024 envs of 16x16 at 32 px (805 MB of frames), 4 096 envs of 16x16 at 8 px, 64 envs of 64x64 at 32 px.  For each: the
render call's time by device events (highlight on: a gen_obs into the private buffer + the render kernel; and highlight off: the
render kernel alone), with non-temporal and with plain 16-byte stores (MGX_RENDER_STORES), frames per second and the frame bytes
written over the highlight-off time -- to set against the 6.0-6.2 TB/s an MI355X sustains for plain streaming stores.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from multigrid_amd import BatchedMultiGridEnv, EnvSpec  # noqa: E402
from tests import util  # noqa: E402

CASES = [("16x16_b1024_ts32", EnvSpec(16, 16, 4, 7, max_steps=1024), 1024, 32),
         ("16x16_b4096_ts8", EnvSpec(16, 16, 4, 7, max_steps=1024), 4096, 8),
         ("64x64_b64_ts32", EnvSpec(64, 64, 16, 9, max_steps=1 << 14), 64, 32)]


def time_render(env, ts, highlight, out, iters):
    for _ in range(3):
        env.render(tile_size=ts, highlight=highlight, out=out)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        env.render(tile_size=ts, highlight=highlight, out=out)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "render_bench needs a HIP device"
    lines = []
    for name, spec, B, ts in CASES:
        st = util.random_state(spec, B, seed=1)
        env = BatchedMultiGridEnv(spec, B, "cuda:0")
        env.load_state(st["grid"], st["agents"], st["rng"], st["target"], st["step_count"], validate=False)
        out = torch.empty((B, spec.height * ts, spec.width * ts, 3), dtype=torch.uint8, device="cuda:0")
        nbytes = out.numel()
        for stores in ("nt", "plain", "nt", "plain"):                    # alternated, twice
            os.environ["MGX_RENDER_STORES"] = stores
            t_off = time_render(env, ts, False, out, args.iters)
            t_on = time_render(env, ts, True, out, args.iters)
            rec = dict(case=name, stores=stores, envs=B, tile_size=ts, frame_bytes=nbytes, render_s=t_off, render_highlight_s=t_on,
                       frames_per_s=B / t_on, write_tb_s=nbytes / t_off / 1e12, share_of_6p1_tb_s=nbytes / t_off / 6.1e12)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        del env, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
