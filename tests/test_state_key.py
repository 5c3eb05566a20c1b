"""State and observation keys (include/mgx.h "STATE KEYS", BatchedMultiGridEnv.state_key / obs_key, EnvSnapshot.state_key) without a GPU.

`model_state_key` / `model_obs_key` state the rule in NumPy, from include/mgx.h alone: the cells go through the library's own
unpacking (layouts.unpack_cells / unpack_cells8) to the triples the rule is written in.  csrc/mgx_state_key.h -- the statement the
kernels are compiled from -- is built by g++ into a stand-alone program, once plain and once under the address and undefined-
behaviour sanitizers, and must give the model's keys.  The host logic of the three methods is driven through `KeyOracle`, the oracle
launcher of tests/test_env_snapshot.py plus a `state_key` / `obs_key` that ARE the model.  tests/test_state_key_gpu.py holds the
kernels to the same model bit for bit."""
import ctypes as C
import gc
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib, layouts
from multigrid_amd.constants import Type
from tests.test_env_snapshot import CopyOracle, make_env
from tests.test_episode_stats import actions_for, empty_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
U64 = np.uint64
STEP, RNG = 1, 2                                                            # MGX_KEY_STEP_COUNT, MGX_KEY_RNG
SALTS = (0, 0xC3A5C85C97CB3127 | (1 << 63))                                 # (the second one: >= 2**63)


# ---- the rule, in NumPy ------------------------------------------------------------------------------------------------------------

def splitmix64(x):
    x = np.atleast_1d(np.asarray(x, dtype=U64)).copy()
    x += U64(0x9E3779B97F4A7C15)                                            # (array arithmetic on uint64: mod 2^64, silently)
    x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
    return x ^ (x >> U64(31))


def terms(tag, idx, payload, salt):
    """splitmix64(w ^ salt), w = tag << 60 | idx << 32 | payload, over arrays"""
    w = (U64(tag) << U64(60)) | (np.asarray(idx).astype(U64) << U64(32)) | np.asarray(payload).astype(U64)
    return splitmix64((w ^ U64(salt)).reshape(-1)).reshape(w.shape)


def xor_all(t):
    return np.bitwise_xor.reduce(t, axis=-1)


def cell_bytes_of(spec):
    return spec.cell_bytes if spec.cell_bytes in (1, 3) else 2


def triples_of(cb, cells):
    """what `BatchedMultiGridEnv.grid` shows of the cells: u8[n,H*W,3]"""
    cells = np.asarray(cells)
    tri = cells if cb == 3 else (layouts.unpack_cells8(cells) if cb == 1 else layouts.unpack_cells(cells))
    return tri.reshape(cells.shape[0], -1, 3)


def cell_terms(tri, salt):
    """tag 1 over triples u8[n,HW,3]: the XOR of the cell words of every row"""
    tri = tri.astype(np.uint32)
    c = (tri[..., 0] & 15) | ((tri[..., 1] & 7) << 4) | (tri[..., 2] << 8)
    if c.shape[1] % 2:
        c = np.concatenate([c, np.full((c.shape[0], 1), 0xFFFF, np.uint32)], axis=1)
    payload = c[:, 0::2] | (c[:, 1::2] << 16)
    return xor_all(terms(1, np.arange(payload.shape[1]), payload, salt))


def model_state_key(cb, cells, agents, rng, step_count, aux, flags=0, salt=0):
    """keys u64[n] of n rows: cells [n,...] in the format `cb`, agents u8[n,A,8], rng 64-bit [n,4], step_count i32[n], aux u8[n,16]
    or None"""
    n = np.asarray(cells).shape[0]
    key = cell_terms(triples_of(cb, cells), salt)
    ag = np.ascontiguousarray(agents, dtype=np.uint8).reshape(n, -1).view("<u4")
    key ^= xor_all(terms(2, np.arange(ag.shape[1]), ag, salt))
    ax = np.zeros((n, 4), np.uint32) if aux is None else np.ascontiguousarray(aux, dtype=np.uint8).reshape(n, 16).view("<u4")
    key ^= xor_all(terms(3, np.arange(4), ax, salt))
    if flags & STEP:
        key ^= terms(4, 0, np.asarray(step_count).astype(np.int64) & 0xFFFFFFFF, salt)
    if flags & RNG:
        w = np.ascontiguousarray(rng).view(U64).reshape(n, 4)
        halves = np.stack([w & U64(0xFFFFFFFF), w >> U64(32)], axis=-1).reshape(n, 8)
        key ^= xor_all(terms(5, np.arange(8), halves, salt))
    return key


def model_obs_key(obs, dirs, salt=0):
    """keys u64[...] of views obs u8[...,v,v,3] / dirs u8[...]"""
    obs, dirs = np.asarray(obs), np.asarray(dirs)
    flat = obs.reshape(dirs.size, -1)
    pad = (-flat.shape[1]) % 4
    words = np.ascontiguousarray(np.concatenate([flat, np.zeros((flat.shape[0], pad), np.uint8)], axis=1)).view("<u4")
    key = xor_all(terms(8, np.arange(words.shape[1]), words, salt)) ^ terms(9, 0, dirs.reshape(-1), salt)
    return key.reshape(dirs.shape)


def check_the_mixer():
    """the issue's check value, and a worked word by Python's integers"""
    assert int(splitmix64(0)[0]) == 0xE220A8397B1DCDAF
    assert int(terms(0, 0, 0, 0)) == 0xE220A8397B1DCDAF
    x = ((4 << 60 | 7) ^ 1) + 0x9E3779B97F4A7C15 & (2 ** 64 - 1)           # tag 4, idx 0, payload 7, salt 1
    x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9 & (2 ** 64 - 1)
    x = (x ^ x >> 27) * 0x94D049BB133111EB & (2 ** 64 - 1)
    assert int(terms(4, 0, 7, 1)) == x ^ x >> 31


# ---- random states -----------------------------------------------------------------------------------------------------------------

def valid_triples(contents=True):
    """every (type, colour, state byte) the 16-bit format holds with the reference's ranges -- types 0..10, colours 0..5, states
    0..3, a box's content (kind 1..7, colour 0..5) in the state byte -- u8[K,3]; contents=False: what the compact format holds too"""
    out = []
    for t in range(11):
        for c in range(6):
            if contents:
                sbs = list(range(4))
                if t == int(Type.box):
                    sbs += [s | kind << 2 | cc << 5 for s in range(4) for kind in range(1, 8) for cc in range(6)]
            else:
                sbs = list(range(3)) if t == int(Type.door) else ([0, 1, 2, 3] if t == int(Type.agent) else [0])
            out += [(t, c, sb) for sb in sbs]
    return np.array(out, dtype=np.uint8)


def random_rows(r, n, W, H, A, cb):
    """n random VALID states as the model and the host program take them (cells in the format cb)"""
    tri = valid_triples(contents=cb != 1)
    g = tri[r.integers(0, len(tri), size=(n, H, W))]
    cells = g if cb == 3 else (layouts.pack_cells8(g) if cb == 1 else layouts.pack_cells(g))
    return {"cells": np.ascontiguousarray(cells), "agents": r.integers(0, 256, size=(n, A, 8), dtype=np.uint8),
            "rng": r.integers(0, 2 ** 64, size=(n, 4), dtype=U64), "step_count": r.integers(-5, 2 ** 31 - 1, size=n).astype(np.int32),
            "aux": r.integers(0, 256, size=(n, 16), dtype=np.uint8)}


def keys_of(cb, rows, flags=0, salt=0, aux=True):
    return model_state_key(cb, rows["cells"], rows["agents"], rows["rng"], rows["step_count"], rows["aux"] if aux else None, flags, salt)


# ---- csrc/mgx_state_key.h, built by g++ into a program of its own ------------------------------------------------------------------

HOST_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "mgx_state_key.h"
#include "mgx_aux_geom.h"
using namespace mgx;
static long long rd(FILE *f) { long long v = 0; if (fread(&v, 8, 1, f) != 1) return -1; return v; }
static std::vector<uint8_t> bytes(FILE *f, size_t n) {
    std::vector<uint8_t> b(n);
    if (n && fread(b.data(), 1, n, f) != n) { printf("short input\n"); exit(2); }
    return b;
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    printf("mix %016llx\n", (unsigned long long)key_mix(0));
    for (uint32_t p = 0; p < 65536; ++p) {                 // two 16-bit cells at once = one after the other
        const uint32_t q = (p * 40503u + 77u) & 0xffffu;
        if (key_pair16(p | q << 16) != (key_cell16(p) | key_cell16(q) << 16)) { printf("FAILED key_pair16 %x %x\n", p, q); return 1; }
        uint32_t w0, w1;                                  // four compact cells at once
        key_quad8(p | q << 16, w0, w1);
        if (w0 != (key_cell8(p) | key_cell8(p >> 8) << 16) || w1 != (key_cell8(q) | key_cell8(q >> 8) << 16)) { printf("FAILED key_quad8 %x %x\n", p, q); return 1; }
    }
    for (long long kind; (kind = rd(f)) >= 0;) {
        if (kind == 0) {                                   // states: W H A cb n has_aux nq, the queries, the members
            const int W = (int)rd(f), H = (int)rd(f), A = (int)rd(f), cb = (int)rd(f), n = (int)rd(f), has_aux = (int)rd(f), nq = (int)rd(f);
            std::vector<unsigned long long> q(2 * nq);
            for (auto &v : q) v = (unsigned long long)rd(f);
            const size_t tile = (size_t)W * H * cb;
            const auto cells = bytes(f, tile * n), agents = bytes(f, (size_t)n * A * 8), rng = bytes(f, (size_t)n * 32),
                       sc = bytes(f, (size_t)n * 4), aux = bytes(f, has_aux ? (size_t)n * 16 : 0);
            for (int k = 0; k < nq; ++k)
                for (int i = 0; i < n; ++i) {
                    std::vector<uint8_t> tile_i(cells.begin() + i * tile, cells.begin() + (i + 1) * tile);   // (its own allocation:
                    uint64_t words[4];                                                                        //  an over-read shows)
                    for (int w = 0; w < 4; ++w) { words[w] = 0; for (int b = 0; b < 8; ++b) words[w] |= (uint64_t)rng[i * 32 + w * 8 + b] << (8 * b); }
                    const int32_t step = (int32_t)((uint32_t)sc[i * 4] | (uint32_t)sc[i * 4 + 1] << 8 | (uint32_t)sc[i * 4 + 2] << 16 | (uint32_t)sc[i * 4 + 3] << 24);
                    std::vector<uint8_t> ag(agents.begin() + (size_t)i * A * 8, agents.begin() + (size_t)(i + 1) * A * 8);
                    std::vector<uint8_t> ax;
                    if (has_aux) ax.assign(aux.begin() + i * 16, aux.begin() + (i + 1) * 16);
                    printf("%016llx\n", (unsigned long long)state_key_host(W, H, A, cb, tile_i.data(), ag.data(), words, step,
                                                                          has_aux ? ax.data() : nullptr, (uint32_t)q[2 * k], q[2 * k + 1]));
                }
        } else if (kind == 1) {                            // views: v n nq, the salts, obs, dir
            const int v = (int)rd(f), n = (int)rd(f), nq = (int)rd(f);
            std::vector<unsigned long long> q(nq);
            for (auto &s : q) s = (unsigned long long)rd(f);
            const size_t row = (size_t)3 * v * v;
            const auto obs = bytes(f, row * n), dir = bytes(f, n);
            for (int k = 0; k < nq; ++k)
                for (int i = 0; i < n; ++i) {
                    std::vector<uint8_t> img(obs.begin() + i * row, obs.begin() + (i + 1) * row);
                    printf("%016llx\n", (unsigned long long)obs_key_host(v, img.data(), dir[i], q[k]));
                }
        } else {                                           // geometry: cb tile n base
            const int cb = (int)rd(f), tile = (int)rd(f);
            const long long n = rd(f), base = rd(f);
            const StateKeyGeom g = state_key_geom(tile, n);
            const int unit = state_key_unit(cb, tile, (uintptr_t)base), chunk = state_key_chunk_bytes(cb, unit);
            if (g.group < 1 || (g.group & (g.group - 1)) || g.group * g.run > 64 || (g.group < 64 && 2 * g.group * g.run <= 64)
                || g.nwaves * g.run < n || (g.nwaves - 1) * g.run >= n || tile % unit || base % unit || chunk % (2 * cb)
                || (unit >= chunk && unit != chunk) || (cb == 3 && chunk != 6)) { printf("FAILED geometry\n"); return 1; }
            printf("%d %d %d %d\n", g.run, g.group, unit, chunk);
        }
    }
    fclose(f);
    return 0;
}
"""

HOST_SHAPES = ((5, 5), (6, 5), (8, 8), (7, 9), (255, 255))
QUERIES = [(flags, salt) for flags in range(4) for salt in SALTS]


def geometry(cb, tile_bytes, n, base=0):
    """(run, group, unit, chunk bytes) of a mgx_state_key launch: csrc/mgx_aux_geom.h restated (held to it below)"""
    run = max(1, min(64, 4096 // tile_bytes))
    while run > 1 and (n + run - 1) // run < 1024:
        run = (run + 1) // 2
    group = 64
    while group * run > 64:
        group //= 2
    unit = 16
    while unit > 1 and (tile_bytes % unit or base % unit):
        unit //= 2
    if cb == 3:
        unit = min(unit, 2)
    return run, group, unit, 6 if cb == 3 else max(unit, 2 * cb)


def _i64(*v):
    return np.array(v, dtype=np.int64).view(np.uint8).tobytes()


def _u64s(v):
    return np.array(v, dtype=U64).tobytes()


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no C++ compiler"
    d = tmp_path_factory.mktemp("state_key_host")
    src = d / "state_key_host.cpp"
    src.write_text(HOST_MAIN)
    inc = ["-I", os.path.join(ROOT, "multigrid_amd", "csrc")]
    exes = {"plain": str(d / "plain"), "sanitized": str(d / "sanitized")}
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-Werror", *inc, str(src), "-o", exes["plain"]])
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           *inc, str(src), "-o", exes["sanitized"]])

    def run(which, payload: bytes):
        path = d / f"input_{which}.bin"
        path.write_bytes(payload)
        p = subprocess.run([exes[which], str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines = p.stdout.split("\n")
        assert lines[0] == "mix e220a8397b1dcdaf"
        return [ln for ln in lines[1:] if ln]
    return run


@pytest.fixture(scope="module")
def host_cases():
    """(payload, expected key lines) over the shapes, agent counts, formats, flags and salts"""
    r = np.random.default_rng(11)
    payload, want = [], []
    for W, H in HOST_SHAPES:
        for A in (1, 3, 32):
            for cb in (2, 1, 3):
                n = 1 if W == 255 else 3
                has_aux = (A + cb) % 2                                       # (a set without aux: in half of the cases)
                rows = random_rows(r, n, W, H, A, cb)
                payload.append(_i64(0, W, H, A, cb, n, has_aux, len(QUERIES)) + _u64s([v for q in QUERIES for v in q]))
                payload += [rows[m].tobytes() for m in ("cells", "agents", "rng", "step_count")] + ([rows["aux"].tobytes()] if has_aux else [])
                for flags, salt in QUERIES:
                    want += [f"{int(k):016x}" for k in keys_of(cb, rows, flags, salt, aux=bool(has_aux))]
    for v in (3, 7, 15):
        obs, dirs = r.integers(0, 256, size=(5, v, v, 3), dtype=np.uint8), r.integers(0, 4, size=5, dtype=np.uint8)
        payload += [_i64(1, v, 5, len(SALTS)) + _u64s(SALTS), obs.tobytes(), dirs.tobytes()]
        for salt in SALTS:
            want += [f"{int(k):016x}" for k in model_obs_key(obs, dirs, salt)]
    return b"".join(payload), want


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_header_gives_the_models_keys(host_programs, host_cases, which):
    check_the_mixer()                                                       # (the program prints key_mix(0): `host_programs` holds it
    payload, want = host_cases                                              #  to the same value)
    got = host_programs(which, payload)
    assert len(got) == len(want) == (4 * 9 * 3 + 9 * 1) * len(QUERIES) + 3 * 5 * len(SALTS)
    assert got == want


def test_the_launch_geometry_is_what_the_gpu_tests_name(host_programs):
    cases = [(cb, W * H * cb, n, base) for W, H in HOST_SHAPES + ((64, 64), (6, 6)) for cb in (1, 2, 3)
             for n in (1, 63, 65, 67, 1023, 1025, 8191, 65535, 65537, 1 << 20) for base in (4096, 4097, 4098, 4100, 4104)
             if not (cb == 2 and base % 2)]
    got = host_programs("sanitized", b"".join(_i64(2, *c) for c in cases))
    assert [tuple(int(v) for v in ln.split()) for ln in got] == [geometry(*c) for c in cases]


# ---- what a key depends on: asked of the HEADER (state_key_host, by the stand-alone program), and of the model beside it ------------

MEMBERS = ("cells", "agents", "rng", "step_count", "aux")


def stack(states):
    return {m: np.concatenate([st[m] for st in states]) for m in MEMBERS}


@pytest.fixture(params=["plain", "sanitized"])
def header_keys(request, host_programs):
    """keys(W, H, A, cb, rows, queries, aux=True) -> u64[len(queries), n]: state_key_host's keys of the stacked rows for every
    (flags, salt) of `queries`, read from the program's output -- and equal to the model's"""
    def keys(W, H, A, cb, rows, queries, aux=True):
        n = rows["cells"].shape[0]
        assert rows["cells"].reshape(n, -1).shape[1] * rows["cells"].itemsize == W * H * cb and rows["agents"].shape[1] == A
        payload = [_i64(0, W, H, A, cb, n, int(aux), len(queries)) + _u64s([v for q in queries for v in q])]
        payload += [np.ascontiguousarray(rows[m]).tobytes() for m in MEMBERS[:4]] + ([rows["aux"].tobytes()] if aux else [])
        lines = host_programs(request.param, b"".join(payload))
        got = np.array([int(ln, 16) for ln in lines], dtype=U64).reshape(len(queries), n)
        for k, (flags, salt) in enumerate(queries):
            assert (got[k] == keys_of(cb, rows, flags, salt, aux)).all(), (cb, flags, salt)
        return got
    return keys


def test_the_key_does_not_depend_on_the_cell_format(header_keys):
    r = np.random.default_rng(3)
    queries = [(STEP | RNG, SALTS[1]), (0, 0)]
    for W, H in ((5, 5), (6, 5), (7, 9)):
        tri = valid_triples(contents=False)
        g = tri[r.integers(0, len(tri), size=(40, H, W))]
        rows = random_rows(r, 40, W, H, 3, 3)
        by_format = [header_keys(W, H, 3, cb, dict(rows, cells=cells), queries)
                     for cb, cells in ((2, layouts.pack_cells(g)), (1, layouts.pack_cells8(g)), (3, g))]
        assert (by_format[0] == by_format[1]).all() and (by_format[0] == by_format[2]).all()
        assert len(np.unique(by_format[0][0])) == len(np.unique(by_format[0][1])) == 40


def cell_edits(t, c, sb, compact):
    """the triples that differ from (t, c, sb) in ONE field -- type, colour, state, a box's content -- and that the format holds"""
    box, door, agent = int(Type.box), int(Type.door), int(Type.agent)
    s, kind, cc = sb & 3, (sb >> 2) & 7, sb >> 5
    out = [(t, (c + 1) % 6, sb)]                                             # colour
    if compact:
        if s == 0:
            out.append(((t + 1) % 11, c, 0))                                 # type (every type holds state 0)
        elif s < 3:
            out.append((door if t == agent else agent, c, s))               # type: door <-> agent overlay keep a state 1, 2
        if t == door:
            out.append((t, c, (s + 1) % 3))                                  # state
        elif t == agent:
            out.append((t, c, (s + 1) % 4))
        return out
    if t != box:
        t2 = (t + 1) % 11
        return out + [(t2 if t2 != box else 8, c, sb), (t, c, (sb + 1) % 4)]   # type, state
    out += [(int(Type.key), c, s), (t, c, sb ^ 1), (t, c, s | (kind % 7 + 1) << 2 | cc << 5)]   # type, state, content kind
    if kind:
        out += [(t, c, s | kind << 2 | (cc + 1) % 6 << 5), (t, c, s)]        # content colour, no content
    return out


@pytest.mark.parametrize("cb", [2, 1, 3])
def test_every_field_of_the_state_changes_the_key(header_keys, cb):
    r = np.random.default_rng(4 + cb)
    W, H, A = 5, 5, 3
    pack = {1: layouts.pack_cells8, 2: layouts.pack_cells, 3: lambda g: g}[cb]
    base = random_rows(r, 1, W, H, A, 3)
    g = valid_triples(contents=cb != 1)[r.integers(0, len(valid_triples(contents=cb != 1)), size=(1, H, W))]
    if cb != 1:
        g[0, 2, 2] = (int(Type.box), 3, 1 | 2 << 2 | 4 << 5)                 # a box with a content, somewhere in the middle
    base["cells"] = pack(g)
    states, kinds = [base], ["base"]

    def add(kind, **changed):
        states.append(dict(base, **changed))
        kinds.append(kind)
    for y in range(H):
        for x in range(W):
            for e in cell_edits(*(int(v) for v in g[0, y, x]), compact=cb == 1):
                g2 = g.copy()
                g2[0, y, x] = e
                add("field", cells=pack(g2))
    for m in ("agents", "aux"):
        flat = base[m].reshape(-1)
        for j in range(flat.size):
            for bit in (1, 0x80):
                other = flat.copy()
                other[j] ^= bit
                add("field", **{m: other.reshape(base[m].shape)})
    add("step", step_count=base["step_count"] + 1)
    for j in range(4):
        for bit in (0, 31, 32, 63):
            other = base["rng"].copy()
            other[0, j] ^= U64(1) << U64(bit)
            add("rng", rng=other)
    add("same", aux=base["aux"].copy())
    if cb == 2:                                                              # the derived opaque bit is no part of the key
        for y in range(H):
            for x in range(W):
                flipped = base["cells"].copy()
                flipped[0, y, x] ^= 0x8000
                add("same", cells=flipped)
        add("same", cells=base["cells"] ^ 0x8000)
    if cb == 3:                                                              # byte values beyond the packed format: keyed after the masks
        for y in range(H):
            for x in range(W):
                for k, extra in ((0, 0x10), (0, 0xF0), (1, 0x08), (1, 0xF8)):
                    g2 = g.copy()
                    g2[0, y, x, k] |= extra
                    add("same", cells=g2)
    queries = [(flags, 0) for flags in range(4)] + [(0, 1), (0, SALTS[1])]
    K = header_keys(W, H, A, cb, stack(states), queries)
    kinds = np.array(kinds)
    assert (kinds == "field").sum() > 25 * 2 + 2 * (A * 8 + 16)
    for flags in range(4):
        differs = K[flags] != K[flags, 0]
        assert differs[kinds == "field"].all(), (flags, np.flatnonzero((kinds == "field") & ~differs)[:5])
        assert (differs[kinds == "step"] == bool(flags & STEP)).all() and (differs[kinds == "rng"] == bool(flags & RNG)).all()
        assert not differs[kinds == "same"].any(), (flags, np.flatnonzero((kinds == "same") & differs)[:5])
    assert len({int(K[q, 0]) for q in range(len(queries))}) == len(queries)  # every flag combination and every salt: another key
    # a set without aux is keyed as sixteen zero bytes
    zero = dict(base, aux=np.zeros((1, 16), np.uint8))
    assert (header_keys(W, H, A, cb, zero, queries) == header_keys(W, H, A, cb, base, queries, aux=False)).all()


def test_the_missing_last_cell_of_an_odd_grid_is_0xffff(header_keys):
    """25 cells end in half a word whose other half is 0xFFFF -- no cell's canonical value (bit 7 of one is always 0).  The same
    25 cells followed by a 26th, as a 13x2 grid of byte triples, differ from the 5x5 grid in word 12 alone: the XOR of the two
    keys is the XOR of that word's two terms, which pins the pad."""
    r = np.random.default_rng(6)
    base = random_rows(r, 4, 5, 5, 2, 3)
    queries = [(0, 0), (STEP | RNG, SALTS[1])]
    for cb in (3, 2, 1):
        if cb == 1:
            tri = valid_triples(contents=False)
            base = dict(base, cells=tri[r.integers(0, len(tri), size=(4, 5, 5))])
        cells = {3: lambda g: g, 2: layouts.pack_cells, 1: layouts.pack_cells8}[cb](base["cells"])
        odd = header_keys(5, 5, 2, cb, dict(base, cells=cells), queries)
        flat = base["cells"].reshape(4, 25, 3).astype(np.uint32)
        c24 = (flat[:, 24, 0] & 15) | ((flat[:, 24, 1] & 7) << 4) | (flat[:, 24, 2] << 8)
        for last in ((15, 7, 255), (0, 0, 0), (1, 0, 0)):
            c25 = (last[0] & 15) | (last[1] & 7) << 4 | last[2] << 8
            even = np.concatenate([base["cells"].reshape(4, 25, 3), np.broadcast_to(np.array(last, np.uint8), (4, 1, 3))], axis=1)
            even = header_keys(13, 2, 2, 3, dict(base, cells=np.ascontiguousarray(even.reshape(4, 2, 13, 3))), queries)
            for k, (_, salt) in enumerate(queries):
                assert ((odd[k] ^ even[k]) == (terms(1, 12, c24 | 0xFFFF << 16, salt) ^ terms(1, 12, c24 | c25 << 16, salt))).all(), (cb, last)
                assert (odd[k] != even[k]).all()


def test_distinct_states_have_distinct_keys(header_keys):
    """every one-cell edit of a 5x5 state over all valid triples, and 200 000 two-cell edits: as many keys as states (salt 0)"""
    r = np.random.default_rng(5)
    tri = valid_triples()
    assert len(tri) == 10 * 6 * 4 + 6 * (4 + 4 * 7 * 6)
    base = tri[r.integers(0, len(tri), size=25)]
    one = np.repeat(base[None], 25 * len(tri), axis=0)
    pos = np.repeat(np.arange(25), len(tri))
    one[np.arange(len(one)), pos] = np.tile(tri, (25, 1))
    two = np.repeat(base[None], 200_000, axis=0)
    for _ in range(2):
        two[np.arange(len(two)), r.integers(0, 25, size=len(two))] = tri[r.integers(0, len(tri), size=len(two))]
    states = np.concatenate([one, two])
    n_states = len(np.unique(states.reshape(len(states), -1), axis=0))
    assert n_states > 25 * (len(tri) - 1) + 150_000
    fixed = random_rows(r, 1, 5, 5, 2, 3)
    rows = {m: np.repeat(fixed[m], len(states), axis=0) for m in MEMBERS}
    rows["cells"] = states.reshape(len(states), 5, 5, 3)
    keys = header_keys(5, 5, 2, 3, rows, [(0, 0)])[0]
    assert len(np.unique(keys)) == n_states
    # ... and so in the 16-bit cells
    keys16 = header_keys(5, 5, 2, 2, dict(rows, cells=layouts.pack_cells(rows["cells"])), [(0, 0)])[0]
    assert (keys16 == keys).all()


# ---- the Python layer over the model -----------------------------------------------------------------------------------------------

class KeyOracle(CopyOracle):
    """the oracle launcher + env_copy (the model of tests/test_env_snapshot.py) + state_key / obs_key, which are the model above;
    `key_calls` records (what, n, members, flags, salt)."""

    def __init__(self, spec):
        super().__init__(spec)
        self.key_calls = []

    def state_key(self, n, rows, n_rows, idx, flags, salt, keys, bad):
        self.key_calls.append(("state", n, sorted(k for k, v in rows.items() if v is not None), flags, salt))
        r = self._np(rows)
        for i in range(n):
            s = i if idx is None else int(idx[i])
            if not 0 <= s < n_rows:
                if bad is not None:
                    bad[0] += 1
                    bad[1] = min(int(bad[1]), min(i, INT32_MAX))
                continue
            k = model_state_key(cell_bytes_of(self.spec), r["cells"][s:s + 1], r["agents"][s:s + 1], r["rng"][s:s + 1],
                                r["step_count"][s:s + 1], r["aux"][s:s + 1] if "aux" in r else None, flags, salt)
            keys[i] = int(k.view(np.int64)[0])

    def obs_key(self, n, obs, dir, salt, keys):
        self.key_calls.append(("obs", n, None, 0, salt))
        assert n == dir.numel() == keys.numel()
        keys.copy_(torch.from_numpy(model_obs_key(obs.numpy(), dir.numpy(), salt).view(np.int64)))


SPEC = EnvSpec(5, 5, 2, 3, max_steps=6)


def env_keys(env, flags=0, salt=0):
    """the model on what the env shows: .grid (byte triples), agents, aux, step_count, rng"""
    return model_state_key(3, env.grid.cpu().numpy(), env.agents.cpu().numpy(), env.rng.cpu().numpy(), env.step_count.cpu().numpy(),
                           env.aux.cpu().numpy(), flags, salt).view(np.int64)


def test_state_key_of_a_batch_and_its_arguments():
    B = 7
    be = KeyOracle(SPEC)
    env = make_env("pool", B=B, backend=be)
    for a in actions_for(B, 2, 3, 4):
        env.step(a, auto_reset=True)
    keys = env.state_key()
    assert keys.dtype is torch.int64 and tuple(keys.shape) == (B,) and keys.device == env.device
    assert keys.numpy().tolist() == env_keys(env).tolist()
    assert be.key_calls[-1] == ("state", B, ["agents", "aux", "cells", "rng", "step_count"], 0, 0)
    for kw, flags in (({"step_count": True}, STEP), ({"rng": True}, RNG), ({"step_count": True, "rng": True}, STEP | RNG)):
        got = env.state_key(salt=SALTS[1], **kw)
        assert got.numpy().tolist() == env_keys(env, flags, SALTS[1]).tolist() and be.key_calls[-1][3:] == (flags, SALTS[1])
        assert (got != keys).all()
    # chosen envs, repeats allowed; out= is written and handed back
    ids = torch.tensor([6, 0, 0, 3])
    out = torch.full((4,), 77, dtype=torch.int64)
    assert env.state_key(ids, out=out) is out and out.tolist() == keys[ids].tolist()
    assert env.state_key(torch.zeros(0, dtype=torch.int64)).shape == (0,)
    # refusals
    for salt in (-1, 2 ** 64, 1.0, True, None):
        with pytest.raises(ValueError, match=r"salt must be an int in \[0, 2\*\*64\)"):
            env.state_key(salt=salt)
        with pytest.raises(ValueError, match=r"salt must be an int in \[0, 2\*\*64\)"):
            env.obs_key(salt=salt)
    env.state_key(salt=2 ** 64 - 1)
    for t in (torch.arange(4, dtype=torch.int32), torch.arange(4).reshape(2, 2), torch.arange(8)[::2], [0, 1]):
        with pytest.raises(ValueError, match="env_ids must be a contiguous int64 tensor"):
            env.state_key(t)
    for bad_out in (torch.zeros(B, dtype=torch.int32), torch.zeros(B + 1, dtype=torch.int64), torch.zeros(2 * B, dtype=torch.int64)[::2],
                    np.zeros(B, np.int64)):
        with pytest.raises(ValueError, match="out= must be a contiguous int64 tensor of shape"):
            env.state_key(out=bad_out)
    with pytest.raises(ValueError, match="out= must be a contiguous int64 tensor of shape"):
        env.state_key(ids, out=torch.zeros(B, dtype=torch.int64))
    env._session = object()
    with pytest.raises(RuntimeError, match="persistent session"):
        env.state_key()
    env._session = None
    with pytest.raises(RuntimeError, match="no state loaded"):
        BatchedMultiGridEnv(SPEC, B, "cpu", backend=KeyOracle(SPEC)).state_key()
    with pytest.raises(RuntimeError, match="sub-shard of split"):
        env.split(2)[0].state_key()
    # ids out of range: their keys are left alone, and check_errors() tells -- in the words it has for snapshots
    out = torch.full((4,), 77, dtype=torch.int64)
    env.state_key(torch.tensor([1, B, -1, 2]), out=out)
    assert out.tolist() == [int(keys[1]), 77, 77, int(keys[2])]
    with pytest.raises(ValueError, match=r"2 pair\(s\) named an env id or a snapshot row out of range.*first at pair 1"):
        env.check_errors()
    env.check_errors()


def test_forks_and_restores_have_their_sources_keys():
    B = 130
    env = make_env("pool", B=B, backend=KeyOracle(SPEC))
    for a in actions_for(B, 2, 3, 4):
        env.step(a, auto_reset=True)
    before = env.state_key(step_count=True, rng=True)
    assert len(torch.unique(before)) > B // 2
    src, dst = torch.tensor([5, 5, 64, 129]), torch.tensor([0, 7, 5, 100])
    env.fork(src, dst)
    after = env.state_key(step_count=True, rng=True)
    assert after[dst].tolist() == before[src].tolist()
    keep = np.setdiff1d(np.arange(B), dst.numpy())
    assert after[keep].tolist() == before[keep].tolist()
    assert len(torch.unique(after[torch.tensor([0, 7, 5])])) == 2            # the dedup: two forks of env 5 and one of env 64
    # snapshot, step on, restore: the key is back, and the snapshot's own key is that key
    snap = env.snapshot()
    at_snap = env.state_key(step_count=True)
    for a in actions_for(B, 2, 2, 9):
        env.step(a, auto_reset=True)
    moved = env.state_key(step_count=True)
    assert (moved != at_snap).all()                                           # (the step count alone sees to that)
    assert snap.state_key(step_count=True).tolist() == at_snap.tolist()
    rows = torch.tensor([3, 3, 129])
    out = torch.zeros(3, dtype=torch.int64)
    assert snap.state_key(rows, step_count=True, out=out) is out and out.tolist() == at_snap[rows].tolist()
    assert env.backend.key_calls[-1][2] == ["agents", "aux", "cells", "rng", "step_count"]
    env.restore(snap)
    assert env.state_key(step_count=True).tolist() == at_snap.tolist()
    # a snapshot row out of range is reported by the env that took the snapshot
    snap.state_key(torch.tensor([0, B]))
    with pytest.raises(ValueError, match=r"1 pair\(s\) named an env id or a snapshot row out of range.*first at pair 1"):
        env.check_errors()
    with pytest.raises(ValueError, match="rows must be a contiguous int64 tensor"):
        snap.state_key(torch.arange(3, dtype=torch.int32))
    # a snapshot whose env is gone has nobody to make the launch
    del env
    gc.collect()
    with pytest.raises(RuntimeError, match="the env this snapshot was taken from is gone"):
        snap.state_key()


def test_the_layout_marker_stays_armed_across_a_key():
    B = 7
    env = make_env("pool", B=B, backend=KeyOracle(SPEC), pool_size=1)        # one layout: the restart marks every env 0, armed
    assert env._tracks() and env._mark["armed"] and env._marker.tolist() == [0] * B
    env.state_key()
    env.state_key(torch.tensor([1, 2]), step_count=True, rng=True)
    assert env._mark["armed"] and env._marker.tolist() == [0] * B
    env.cells                                                                # (what the public tensor costs, for contrast)
    assert not env._mark["armed"] and env._marker.tolist() == [-1] * B


def test_engine_state_is_no_part_of_a_key():
    B = 7
    env = make_env("gen", B=B, backend=KeyOracle(SPEC))
    stats = env.track_episodes()
    for a in actions_for(B, 2, 2, 4):
        env.step(a, auto_reset=True)
    before = env.state_key(step_count=True, rng=True)
    snap_before = env.snapshot().state_key(step_count=True, rng=True)
    assert before.tolist() == snap_before.tolist()
    env._marker.fill_(5)                                                     # the layout marker,
    env.episode.add_(3)                                                      # the restart counter,
    env._gen["gen_state"].add_(1)                                            # the generator's words
    stats.cur_return.add_(1.5); stats.cur_length.add_(2); stats.over.fill_(1)   # and the running episode
    assert env.state_key(step_count=True, rng=True).tolist() == before.tolist()
    snap = env.snapshot()
    assert {"marker", "episode", "gen_state", "cur_return"} <= set(snap.tensors)
    assert snap.state_key(step_count=True, rng=True).tolist() == before.tolist()
    assert env.backend.key_calls[-1][2] == ["agents", "aux", "cells", "rng", "step_count"]


def test_sixteen_bit_and_compact_envs_in_step_have_equal_keys():
    B, T = 7, 8
    envs = []
    for cb in (2, 1):
        spec = EnvSpec(5, 5, 2, 3, max_steps=6, cell_bytes=cb)
        env = BatchedMultiGridEnv(spec, B, "cpu", backend=KeyOracle(spec))
        pg, pa = empty_pool(spec)
        env.load_state(pg[0], pa[0])
        env.seed(3)
        envs.append(env)
    assert envs[0]._cells.dtype is torch.int16 and envs[1]._cells.dtype is torch.uint8
    seen = set()
    for a in actions_for(B, 2, T, 2):
        keys = [env.state_key(step_count=True, rng=True, salt=5) for env in envs]
        assert keys[0].tolist() == keys[1].tolist() == env_keys(envs[0], STEP | RNG, 5).tolist()
        seen |= set(envs[0].state_key().tolist())
        for env in envs:
            env.step(a)
    assert len(seen) > T


def test_obs_key_of_the_envs_outputs_and_of_a_rollouts():
    B, A, v = 7, 2, SPEC.view_size
    env = make_env("pool", B=B, backend=KeyOracle(SPEC))
    env.step(actions_for(B, A, 1, 4)[0], auto_reset=True)
    keys = env.obs_key()
    assert keys.dtype is torch.int64 and tuple(keys.shape) == (B, A)
    assert keys.numpy().tolist() == model_obs_key(env.obs.numpy(), env.dir.numpy()).view(np.int64).tolist()
    assert env.obs_key(salt=SALTS[1]).numpy().tolist() == model_obs_key(env.obs.numpy(), env.dir.numpy(), SALTS[1]).view(np.int64).tolist()
    r = np.random.default_rng(2)
    obs = torch.from_numpy(r.integers(0, 256, size=(4, B, A, v, v, 3), dtype=np.uint8))
    dirs = torch.from_numpy(r.integers(0, 4, size=(4, B, A), dtype=np.uint8))
    obs[1, 2, 0], dirs[1, 2, 0] = obs[3, 5, 1], dirs[3, 5, 1]                 # two agents that see the same thing
    out = torch.zeros((4, B, A), dtype=torch.int64)
    assert env.obs_key(obs, dirs, out=out) is out
    assert out.numpy().tolist() == model_obs_key(obs.numpy(), dirs.numpy()).view(np.int64).tolist()
    assert out[1, 2, 0] == out[3, 5, 1] and len(torch.unique(out)) == out.numel() - 1
    dirs[1, 2, 0] ^= 1
    assert env.obs_key(obs, dirs)[1, 2, 0] != out[3, 5, 1]
    with pytest.raises(ValueError, match="pass both obs and dir"):
        env.obs_key(obs)
    # the env's own outputs need a loaded state and no open session; tensors handed in need neither
    empty = BatchedMultiGridEnv(SPEC, B, "cpu", backend=KeyOracle(SPEC))
    with pytest.raises(RuntimeError, match="no state loaded"):
        empty.obs_key()
    assert empty.obs_key(obs, dirs).tolist() == env.obs_key(obs, dirs).tolist()
    env._session = object()
    with pytest.raises(RuntimeError, match="persistent session"):
        env.obs_key()
    env._session = None
    with pytest.raises(ValueError, match=r"obs must have shape \[..., 3, 3, 3\] and dir the leading shape"):
        env.obs_key(obs, dirs[0])
    with pytest.raises(ValueError, match=r"obs must have shape \[..., 3, 3, 3\]"):
        env.obs_key(obs.reshape(4, B, A, v, v * 3), dirs)
    with pytest.raises(ValueError, match="obs must be a contiguous uint8 tensor"):
        env.obs_key(obs.to(torch.int16), dirs)
    with pytest.raises(ValueError, match="dir must be a contiguous uint8 tensor"):
        env.obs_key(obs, dirs.transpose(0, 1))
    with pytest.raises(ValueError, match="out= must be a contiguous int64 tensor of shape"):
        env.obs_key(obs, dirs, out=torch.zeros((B, A), dtype=torch.int64))


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------------

def test_c_abi_argument_validation():
    """what mgx_state_key and mgx_obs_key check of their own; the checks of every row query: tests/test_row_query_abi.py"""
    from tests.test_row_query_abi import INV, UNS, P as p, full, ref
    L = _lib.lib()
    sc = EnvSpec(5, 5, 2, 3, max_steps=4).to_c()

    def K(sc_, n, src, idx=p, flags=3, salt=2 ** 64 - 1, keys=p, bad=p):
        return L.mgx_state_key(ref(sc_), n, ref(src), idx, flags, salt, keys, bad, None)
    a = full()
    for flags in (4, 8, 0x80000000):
        assert K(sc, 4, a, flags=flags) == INV and K(sc, 0, a, flags=flags) == INV
    assert K(sc, 4, a, keys=None) == INV
    assert K(sc, 4, a, keys=p + 4) == INV
    big = EnvSpec(5, 5, 2, 3).to_c()
    big.width, big.height = 1024, 129
    assert K(big, 4, a) == UNS

    def O(sc_, n, obs=p, dirs=p, keys=p):
        return L.mgx_obs_key(ref(sc_), n, obs, dirs, 5, keys, None)
    assert O(None, 4) == INV and O(sc, -1) == INV
    bad = EnvSpec(5, 5, 2, 3).to_c()
    for v in (0, 16):
        bad.view_size = v
        assert O(bad, 0) == INV
    assert O(sc, 0, None, None, None) == 0
    assert O(sc, 4, obs=None) == INV and O(sc, 4, dirs=None) == INV and O(sc, 4, keys=None) == INV and O(sc, 4, keys=p + 4) == INV
    assert O(sc, 4 * 32 * (2 ** 31 - 1) + 1) == UNS                          # (v = 3: 32 views per wavefront)


def test_the_exports_are_the_headers_declarations():
    from tests.test_capi import declared_functions
    names = declared_functions()
    for sym in ("mgx_state_key", "mgx_obs_key"):
        assert sym in names and sym in _lib.EXPORTS and getattr(_lib.lib(), sym) is not None
    assert set(names) == set(_lib.EXPORTS) and _lib.lib().mgx_abi_version() == _lib.ABI_VERSION == 11
    assert (_lib.KEY_STEP_COUNT, _lib.KEY_RNG) == (STEP, RNG)
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "STATE KEYS" in hdr and "MGX_KEY_STEP_COUNT = 1, MGX_KEY_RNG = 2" in hdr
