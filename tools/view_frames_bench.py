#!/usr/bin/env python3
"""View-frame throughput (BatchedMultiGridEnv.render_views -> include/mgx.h mgx_render_views) on the MI355X.

    python tools/view_frames_bench.py [--iters N] [--out profiles/view_frames.txt]

Cases: the workloads C2, C4 and C5 (multigrid_amd/workloads.py) after a few random steps, every agent's view at 8 px a tile:
16 384, 262 144 and 524 288 views, 0.15, 2.47 and 8.15 GB of frames.  For each, by device events: render_views in both layouts
(channels last / first) with non-temporal and with plain 16-byte stores (MGX_RENDER_STORES), alternated twice, as bytes written
per second.  Two baselines in the same run: `render` of the full frames of the same envs at the same tile size without highlight
(the render kernel alone), as bytes written per second, and the composition a user writes in torch today -- atlas[keys], permute,
contiguous -- from keys made beforehand (the gather and the copy are timed, the keys are not).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from multigrid_amd import workloads  # noqa: E402

DEV = "cuda:0"
TS = 8


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters * 1e-3


def torch_keys(obs, dirs, colours):
    """The keys of include/mgx.h "VIEW FRAMES" in torch ops (highlight on), i64[n, v, v] indexed [view][i][j]."""
    t, c, s = (obs[..., k].long() for k in range(3))
    v = obs.shape[-2]
    ok, st = c <= 5, s & 3
    app = torch.zeros_like(t)
    for ty, first, per in ((2, 1, 1), (8, 1, 1), (3, 7, 1), (5, 31, 1), (6, 37, 1), (7, 43, 1)):
        app = torch.where(ok & (t == ty), first + per * c, app)
    app = torch.where(ok & (t == 4) & (st <= 2), 13 + 3 * c + st, app)
    app = torch.where(t == 9, torch.full_like(app, 49), app)
    ov = torch.where((t == 10) & ok, 1 + 4 * c + ((s - (dirs.long() & 3)[:, None, None] + 3) & 3), torch.zeros_like(t))
    col = colours.long()
    ov[:, v // 2, v - 1] = torch.where(col <= 5, 1 + 4 * col + 3, torch.zeros_like(col))
    return (app * 25 + ov) * 2 + (t != 0).long()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="c2,c4,c5")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "view_frames_bench needs a HIP device"
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for name in args.cases.split(","):
        wl = workloads.make(name)
        env = wl.make_env(DEV, auto_reset=False)
        sp, B = wl.spec, wl.batch
        g = torch.Generator(device=DEV)
        g.manual_seed(1)
        for _ in range(8):
            env.step(torch.randint(0, 7, (B, sp.num_agents), dtype=torch.int8, device=DEV, generator=g))
        n, P = B * sp.num_agents, sp.view_size * TS
        nbytes = n * P * P * 3
        rates = {}
        for cf in (False, True):
            out = torch.empty((B, sp.num_agents) + ((3, P, P) if cf else (P, P, 3)), dtype=torch.uint8, device=DEV)
            for stores in ("nt", "plain", "nt", "plain"):                    # alternated, twice
                os.environ["MGX_RENDER_STORES"] = stores
                t = timed(lambda: env.render_views(tile_size=TS, channels_first=cf, out=out), args.iters)
                rates.setdefault(stores, []).append(nbytes / t / 1e12)
                emit(case=name, what="render_views", layout="channels_first" if cf else "channels_last", stores=stores, views=n,
                     frame_bytes=nbytes, seconds=t, views_per_s=n / t, write_tb_s=nbytes / t / 1e12)
            del out
        # baseline 1: the full frames of the same envs at the same tile size, the render kernel alone (no highlight pass)
        full = torch.empty((B, sp.height * TS, sp.width * TS, 3), dtype=torch.uint8, device=DEV)
        base = {}
        for stores in ("nt", "plain", "nt", "plain"):
            os.environ["MGX_RENDER_STORES"] = stores
            t = timed(lambda: env.render(tile_size=TS, highlight=False, out=full), args.iters)
            base.setdefault(stores, []).append(full.numel() / t / 1e12)
            emit(case=name, what="render_full_frames", stores=stores, envs=B, frame_bytes=full.numel(), seconds=t,
                 write_tb_s=full.numel() / t / 1e12)
        del full
        # baseline 2: what a user composes in torch today
        atlas = env.backend.render_atlas(TS)
        keys = torch_keys(env.obs.reshape(n, sp.view_size, sp.view_size, 3), env.dir.reshape(n), env.agents[:, :, 0].reshape(n))
        keys_t = keys.transpose(1, 2).contiguous()                           # [n, j, i]: tile rows top to bottom
        ours = env.render_views(tile_size=TS).reshape(n, P, P, 3)

        def compose():
            return atlas[keys_t].permute(0, 1, 3, 2, 4, 5).contiguous().view(n, P, P, 3)

        same = bool(torch.equal(compose()[:4096], ours[:4096]))
        t = timed(compose, max(2, args.iters // 4))
        emit(case=name, what="torch_gather_permute_contiguous", views=n, frame_bytes=nbytes, seconds=t, write_tb_s=nbytes / t / 1e12,
             equals_render_views=same)
        for stores in ("nt", "plain"):
            emit(case=name, what="ratio_to_full_frames", stores=stores, render_views_tb_s_min=min(rates[stores]),
                 full_frames_tb_s_max=max(base[stores]), ratio_min_over_max=min(rates[stores]) / max(base[stores]),
                 meets_0p8=min(rates[stores]) >= 0.8 * max(base[stores]))
        del env, keys, keys_t, ours, atlas
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
