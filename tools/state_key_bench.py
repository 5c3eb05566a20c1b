#!/usr/bin/env python3
"""What the state keys of a whole batch cost (BatchedMultiGridEnv.state_key -> mgx_state_key, csrc/mgx_state_key.hip).  GPU box.

The kernel alone, on live envs of the benchmark's shapes (every env holds the configuration's first start: the kernel has no
data-dependent path), keys of all B envs without flags:

    C2  Empty-16x16, 4 agents, 16-bit cells (512-byte tiles),   4 096 envs
    C4  the same shape,                                         65 536 envs
    C5  64x64, 16 agents, compact cells (4 096-byte tiles),    32 768 envs
    C2 shape at 1 048 576 envs (HBM-resident: 0.6 GB of state)

Each point against three references measured in the same run, alternating with it, none of them the code under test:
    read    a plain streaming read of the same number of bytes: 16-byte loads XORed together, grid-stride, one store a wavefront
            (mgx_debug_stream_read of the tools' build, lib/libmgx_dbg.so)
    copy_   a plain copy_ of the same number of bytes (read + write), the stream tools/bw_probe.py measures
    torch   the torch-op chain that computes the same keys from env.grid / agents / aux: unpack to byte triples, canonical cells,
            word pairs, splitmix64 in wrapping int64 arithmetic (logical shifts by masks), XOR by pairwise folding

Every candidate is captured as a graph of back-to-back calls (REPS of them; the torch chain: CHAIN_REPS) and timed with device events
over a replay (per call = / calls); PASSES replays after WARM warm ones: the median and the spread (min, max).  The kernel's keys are
compared with the chain's bit for bit before anything is timed.  No time is asserted.

--obs adds the observation keys of the same batch, and decides how mgx_obs_key loads a view (rows of 3 * v * v bytes are
dword-aligned only every fourth view): the product's byte-aligned dword loads against a load per byte, both from the tools' build
(mgx_debug_obs_key_bytes), alternating, their keys compared first.

Usage: python -m multigrid_amd.build --debug-knobs; python tools/state_key_bench.py [--out profiles/state_key.txt] [--obs]"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigrid_amd import BatchedMultiGridEnv, build, workloads  # noqa: E402

REPS, CHAIN_REPS, PASSES, WARM = 20, 2, 15, 3
DEV = torch.device("cuda:0")
POINTS = (("C2 Empty-16x16 A=4 16-bit cells", "c2", 4096), ("C4 Empty-16x16 A=4 16-bit cells", "c4", 65536),
          ("C5 64x64 A=16 compact cells", "c5", 32768), ("C2 shape at 1M envs", "c2", 1 << 20))
MASK = {s: (1 << (64 - s)) - 1 for s in (27, 30, 31)}


def _i64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def mix(x):
    """splitmix64 on int64 tensors: the arithmetic wraps, the shifts are made logical"""
    x = x + _i64(0x9E3779B97F4A7C15)
    x = (x ^ ((x >> 30) & MASK[30])) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ ((x >> 27) & MASK[27])) * _i64(0x94D049BB133111EB)
    return x ^ ((x >> 31) & MASK[31])


def fold(t):
    """XOR over the last axis by pairwise folding"""
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = torch.cat([t, torch.zeros_like(t[..., :1])], dim=-1)
        t = t[..., 0::2] ^ t[..., 1::2]
    return t[..., 0]


def terms(tag, payload):
    idx = torch.arange(payload.shape[-1], device=payload.device, dtype=torch.int64)
    return fold(mix(_i64(tag << 60) | (idx << 32) | payload))


def torch_chain(env):
    """include/mgx.h "STATE KEYS" (no flags, salt 0) in torch ops over what the env shows"""
    g = env.grid.flatten(1, 2).to(torch.int64)
    c = (g[..., 0] & 15) | ((g[..., 1] & 7) << 4) | (g[..., 2] << 8)
    if c.shape[1] % 2:
        c = torch.cat([c, torch.full_like(c[:, :1], 0xFFFF)], dim=1)
    key = terms(1, c[:, 0::2] | (c[:, 1::2] << 16))
    key = key ^ terms(2, env.agents.flatten(1).view(torch.int32).to(torch.int64) & 0xFFFFFFFF)
    return key ^ terms(3, env.aux.view(torch.int32).to(torch.int64) & 0xFFFFFFFF)


def tools_lib():
    """lib/libmgx_dbg.so: the product's kernels + the streaming read and the byte-load switch of mgx_obs_key"""
    L = C.CDLL(build.build_debug_lib())
    L.mgx_debug_stream_read.restype = C.c_int
    L.mgx_debug_stream_read.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.mgx_obs_key.restype = C.c_int
    L.mgx_obs_key.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    return L


def cur_stream():
    return torch.cuda.current_stream(DEV).cuda_stream


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


def summary(res, names, nbytes):
    cells, med = [], {}
    for k in names:
        v = sorted(res[k])
        med[k] = v[len(v) // 2]
        cells.append(f"{k} {med[k]:9.2f} ({v[0]:.2f}, {v[-1]:.2f}) {nbytes / med[k] / 1e3:7.1f} GB/s")
    return cells, med


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"tools/state_key_bench.py on {torch.cuda.get_device_name(0)}: the keys of all B envs (no flags, salt 0); microseconds per call,",
             f"median (min, max) of {PASSES} graph replays of {REPS} calls each ({CHAIN_REPS} for the torch chain) after {WARM} warm ones; GB/s =",
             "the bytes the key reads (cells + agents + aux) over the median.  kernel = mgx_state_key (one launch); read = a read-only",
             "stream of the same bytes (16-byte loads); copy_ = one plain copy_ of the same bytes; torch = the op chain over env.grid /",
             "agents / aux that gives the same keys (checked).  obs_key: dwords = byte-aligned dword loads (the product), bytes = a load per byte.",
             "  The state of the first three points fits the 256 MB Infinity Cache and is read",
             "again by every call, by the kernel and by the references alike; the 1M-env point streams from HBM.", ""]
    L = tools_lib()
    sink = torch.zeros(4 * L.mgx_debug_stream_read_blocks(), dtype=torch.int32, device=DEV)

    def read_of(t):
        nb, ptr, out = t.numel() * t.element_size() // 16 * 16, t.data_ptr(), sink.data_ptr()
        assert ptr % 16 == 0
        return lambda: L.mgx_debug_stream_read(ptr, nb, out, cur_stream())

    for title, name, B in POINTS:
        wl = workloads.make(name, batch=1, global_batch=B)
        env = BatchedMultiGridEnv(wl.spec, B, DEV)
        env.load_state(wl.grid[0], wl.agents[0], validate=False)
        env.agents[:, :, 2:4] += torch.randint(0, 3, (B, wl.spec.num_agents, 2), dtype=torch.uint8, device=DEV)   # (keys that differ)
        nbytes = env._cells.numel() * env._cells.element_size() + env.agents.numel() + env.aux.numel()
        keys = torch.zeros(B, dtype=torch.int64, device=DEV)
        flat_a = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=DEV)
        flat_b = torch.ones((nbytes + 3) // 4, dtype=torch.int32, device=DEV)
        env.state_key(out=keys)
        want = torch_chain(env)
        torch.cuda.synchronize()
        assert torch.equal(keys, want), "the kernel's keys differ from the torch chain's"
        env.check_errors()
        del want
        res = measure({"kernel": graph_of(lambda: env.state_key(out=keys), REPS), "read": graph_of(read_of(flat_a), REPS),
                       "copy_": graph_of(lambda: flat_a.copy_(flat_b), REPS), "torch": graph_of(lambda: torch_chain(env), CHAIN_REPS)})
        cells, med = summary(res, ("kernel", "read", "copy_", "torch"), nbytes)
        lines.append(f"{title}, {B} envs, {nbytes // B} bytes per env, {nbytes / 1e6:.1f} MB, {len(torch.unique(keys))} distinct keys")
        lines += ["  " + c for c in cells]
        lines.append(f"  kernel / read {med['kernel'] / med['read']:5.2f}   kernel / copy_ {med['kernel'] / med['copy_']:5.2f}   "
                     f"torch / kernel {med['torch'] / med['kernel']:7.1f}")
        if "--obs" in sys.argv:                                   # the observation keys of the same batch: [B, A] views
            okeys = torch.zeros((B, wl.spec.num_agents), dtype=torch.int64, device=DEV)
            env.obs.copy_(torch.randint(0, 11, env.obs.shape, dtype=torch.uint8, device=DEV))
            obytes = env.obs.numel() + env.dir.numel()
            oa, ob = torch.zeros((obytes + 3) // 4, dtype=torch.int32, device=DEV), torch.ones((obytes + 3) // 4, dtype=torch.int32, device=DEV)
            sc, n_views, graphs = C.byref(env.backend.sc), B * wl.spec.num_agents, {}
            by_loads = {}
            for what, knob in (("dwords", 0), ("bytes", 1)):      # (the switch is read when the call is made: each graph keeps its kernel)
                out = torch.zeros_like(okeys)
                call = lambda out=out: L.mgx_obs_key(sc, n_views, env.obs.data_ptr(), env.dir.data_ptr(), 0, out.data_ptr(), cur_stream())
                L.mgx_debug_obs_key_bytes(knob)
                graphs[what] = graph_of(call, REPS)
                by_loads[what] = out
            L.mgx_debug_obs_key_bytes(0)
            env.obs_key(out=okeys)
            torch.cuda.synchronize()
            assert torch.equal(by_loads["dwords"], okeys) and torch.equal(by_loads["bytes"], okeys), "the load variants' keys differ"
            graphs.update({"obs_key": graph_of(lambda: env.obs_key(out=okeys), REPS), "read": graph_of(read_of(oa), REPS),
                           "copy_": graph_of(lambda: oa.copy_(ob), REPS)})
            res = measure(graphs)
            cells, med = summary(res, ("obs_key", "dwords", "bytes", "read", "copy_"), obytes)
            lines.append(f"  observation keys of its {B * wl.spec.num_agents} views (v = {wl.spec.view_size}), {obytes / 1e6:.1f} MB:")
            lines += ["    " + c for c in cells]
            lines.append(f"    obs_key / read {med['obs_key'] / med['read']:5.2f}   obs_key / copy_ {med['obs_key'] / med['copy_']:5.2f}   "
                         f"bytes / dwords {med['bytes'] / med['dwords']:5.2f}")
            del okeys, oa, ob
        lines.append("")
        del env, keys, flat_a, flat_b
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
