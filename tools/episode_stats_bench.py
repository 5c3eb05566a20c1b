#!/usr/bin/env python3
"""What episode accounting (BatchedMultiGridEnv.track_episodes, csrc/mgx_stats.hip) costs.  GPU box.

At C4 (Empty-16x16, 4 agents, 65 536 envs, layout-pool auto-reset) and at C2 (4 096 envs), device events, warm runs, three passes:

  (a) a captured graph of 100 steps, tracking off
  (b) the same with tracking on: the accounting kernel behind every step
  (c) tracking off + the torch formulation of the IDENTICAL accounting captured behind every step (`torch_accounting` below: what a
      user writes today -- element-wise launches over [B,A] / [B] tensors)
  (d) the accounting kernel alone: T = 1 (one step's outputs; 100 launches back to back in a graph), and ONE T = 100 launch over
      a rollout's outputs

Conditions (asserted; the exit code says so): (b) - (a) < (c) - (a) on every pass -- a fused launch that loses to a chain of
element-wise launches is a bug, not noise.  (a) is to be held against the same leg of the parent commit (`--only-a` runs on a tree
without the feature).  The books of (b) and (c) after the same steps are compared bit for bit.

Usage: python tools/episode_stats_bench.py [--only-a] [--out profiles/episode_stats.txt]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigrid_amd import workloads  # noqa: E402

T, PASSES, WARM, REPLAYS = 100, 3, 3, 20


def random_actions(steps, batch, agents, device, seed):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return torch.randint(0, 7, (steps, batch, agents), dtype=torch.int8, device=device, generator=g)


def torch_books(B, A, dev):
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    return {"cur_return": z((B, A), torch.float64), "cur_length": z((B,), torch.int32), "over": z((B,), torch.bool),
            "last_return": z((B, A), torch.float64), "last_length": z((B,), torch.int32), "sum_return": z((B, A), torch.float64),
            "sum_length": z((B,), torch.int64), "counts": z((B, 4), torch.int32)}


def torch_accounting(env, st):
    """The rule of include/mgx.h "EPISODE ACCOUNTING" for a step with layout-pool auto-reset (MGX_RESTART_BEFORE) in torch ops,
    in place on `st`.  Returns the number of torch calls it makes (one or more launches each)."""
    rew, term, trunc, wr = env.reward, env.terminated, env.truncated, env.was_reset
    calls = 0

    def op(x):
        nonlocal calls
        calls += 1
        return x

    restarted = op(wr != 0)
    aborted = op(restarted & op(~st["over"]) & op(st["cur_length"] > 0))       # the restart clause
    op(st["counts"][:, 3].add_(aborted))
    op(st["cur_return"].masked_fill_(aborted[:, None], 0.0))
    op(st["cur_length"].masked_fill_(aborted, 0))
    op(st["over"].logical_and_(op(~restarted)))
    live = op(~st["over"])
    op(st["cur_return"].copy_(op(torch.where(live[:, None], op(st["cur_return"] + rew), st["cur_return"]))))
    op(st["cur_length"].add_(live))
    all_term = op(op(term != 0).all(dim=1))
    closing = op(live & op(op(trunc != 0) | all_term))
    c2 = closing[:, None]
    op(st["last_return"].copy_(op(torch.where(c2, st["cur_return"], st["last_return"]))))
    op(st["last_length"].copy_(op(torch.where(closing, st["cur_length"], st["last_length"]))))
    op(st["sum_return"].copy_(op(torch.where(c2, op(st["sum_return"] + st["cur_return"]), st["sum_return"]))))
    op(st["sum_length"].add_(op(torch.where(closing, st["cur_length"], op(torch.zeros_like(st["cur_length"]))))))
    op(st["counts"][:, 0].add_(closing))
    op(st["counts"][:, 1].add_(op(closing & all_term)))
    op(st["counts"][:, 2].add_(op(closing & op(op(st["cur_return"] > 0).any(dim=1)))))
    op(st["cur_return"].masked_fill_(c2, 0.0))
    op(st["cur_length"].masked_fill_(closing, 0))
    op(st["over"].logical_or_(closing))
    return calls


def capture_with_torch_chain(env, actions, st):
    stream = torch.cuda.current_stream(env.device)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(env.device)
    side.wait_stream(stream)
    calls = 0
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for t in range(actions.shape[0]):
                env.step(actions[t], auto_reset=True)
                calls = torch_accounting(env, st)
    stream.wait_stream(side)
    return graph, calls


def time_replays(replay, dev):
    """us per step of `replay` (a graph of T steps): WARM untimed replays, then PASSES timed regions of REPLAYS replays"""
    stream = torch.cuda.current_stream(dev)
    for _ in range(WARM):
        replay()
    out = []
    for _ in range(PASSES):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        ev0.record(stream)
        for _ in range(REPLAYS):
            replay()
        ev1.record(stream)
        torch.cuda.synchronize(dev)
        out.append(ev0.elapsed_time(ev1) * 1e3 / (REPLAYS * T))
    return out


def time_launch(fn, dev, iters=200):
    stream = torch.cuda.current_stream(dev)
    for _ in range(30):
        fn()
    out = []
    for _ in range(PASSES):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        ev0.record(stream)
        for _ in range(iters):
            fn()
        ev1.record(stream)
        torch.cuda.synchronize(dev)
        out.append(ev0.elapsed_time(ev1) * 1e3 / iters)
    return out


def fresh(name, dev):
    env = workloads.make(name).make_env(dev, auto_reset=True)
    return env


def point(name, dev, only_a):
    wl = workloads.make(name)
    B, A = wl.batch, wl.spec.num_agents
    acts = random_actions(T, B, A, dev, 3)
    res = {"workload": name, "envs": B, "agents": A, "graph_steps": T}
    env = fresh(name, dev)
    g = env.capture_steps(acts, auto_reset=True)
    res["a_untracked_us_per_step"] = time_replays(g.replay, dev)
    if only_a:
        return res, True
    # (b) and (c) from the same state, the same number of replays: their books must agree
    env_b, env_c = fresh(name, dev), fresh(name, dev)
    stats = env_b.track_episodes()
    gb = env_b.capture_steps(acts, auto_reset=True)
    res["b_tracked_us_per_step"] = time_replays(gb.replay, dev)
    books = torch_books(B, A, dev)
    gc, calls = capture_with_torch_chain(env_c, acts, books)
    res["c_torch_chain_us_per_step"] = time_replays(gc.replay, dev)
    res["c_torch_calls_per_step"] = calls
    same = all(torch.equal(stats.tensors[n].to(books[n].dtype), books[n]) for n in books)
    res["books_of_b_and_c_equal"] = bool(same)
    res["episodes_closed"] = int(stats.counts[:, 0].sum())
    a, b, c = (res[k] for k in ("a_untracked_us_per_step", "b_tracked_us_per_step", "c_torch_chain_us_per_step"))
    res["b_minus_a_us"] = [y - x for x, y in zip(a, b)]
    res["c_minus_a_us"] = [y - x for x, y in zip(a, c)]
    # (d) the kernel alone
    be = env_b.backend
    account = be.bind_episode_stats(B, env_b.reward, env_b.terminated, env_b.truncated, env_b.was_reset, 1, stats.tensors)
    account()                                             # (loads the kernel before the capture)
    stream, side, g1 = torch.cuda.current_stream(dev), torch.cuda.Stream(dev), torch.cuda.CUDAGraph()
    side.wait_stream(stream)
    with torch.cuda.stream(side):
        with torch.cuda.graph(g1, stream=side):           # T launches back to back in a graph: no host in the loop
            for _ in range(T):
                account()
    stream.wait_stream(side)
    t1 = time_replays(g1.replay, dev)
    res["d_kernel_T1_us"] = t1
    res["d_kernel_T1_eager_us"] = time_launch(account, dev)        # (one ctypes call each: host-bound)
    env_d = fresh(name, dev)
    st_d = env_d.track_episodes()
    out = env_d.rollout(acts, auto_reset=True)
    roll = lambda: be.episode_stats(B, T, out["reward"], out["terminated"], out["truncated"], out["was_reset"], 1, st_d.tensors)
    tT = time_launch(roll, dev, iters=20)
    res["d_kernel_T100_us_per_launch"] = tT
    # traffic: per env-step the inputs (8 A + A + 2 bytes); per env and LAUNCH the running episode in and out (2 (8 A + 5))
    in_bytes, state_bytes = B * (9 * A + 2), B * 2 * (8 * A + 5)
    res["d_bytes_T1"] = in_bytes + state_bytes
    res["d_GBps_T1"] = [(in_bytes + state_bytes) / (u * 1e3) for u in t1]
    res["d_bytes_T100"] = T * in_bytes + state_bytes
    res["d_GBps_T100"] = [(T * in_bytes + state_bytes) / (u * 1e3) for u in tT]
    ok = same and all(x < y for x, y in zip(res["b_minus_a_us"], res["c_minus_a_us"]))
    return res, ok


if __name__ == "__main__":
    only_a = "--only-a" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    dev = torch.device("cuda", 0)
    results, good = [], True
    for name in ("c4", "c2"):
        r, ok = point(name, dev, only_a)
        results.append(r)
        good &= ok
    text = json.dumps({"device": torch.cuda.get_device_name(dev), "points": results, "conditions_hold": bool(good)}, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text + "\n")
    sys.exit(0 if good else 1)
