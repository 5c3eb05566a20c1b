"""Walking-distance fields (include/mgx.h "DISTANCE FIELDS", BatchedMultiGridEnv.distance_field / agent_distance and the two methods
of EnvSnapshot) without a GPU.

`model_distance` states the rule in NumPy, from include/mgx.h alone -- iterated 4-neighbour dilation over the triples the library's
own unpacking gives (layouts.unpack_cells / unpack_cells8).  csrc/mgx_distance.h -- the classification the kernel is compiled from,
and a plain queue flood -- is built by g++ into a stand-alone program, once plain and once under the address and undefined-behaviour
sanitizers; it must give the model's fields on random grids of every cell format, and an exhaustive table in the same program holds
base passability to the `forward` bit of mask_front_bits (csrc/mgx_action_mask.h) with nobody present: the rule the kernels step by.
The engine tie walks the CPU oracle down the field.  The host logic of the four methods is driven through `DistOracle`, the oracle
launcher of tests/test_action_mask.py plus a `distance` that IS the model.  tests/test_distance_gpu.py holds the kernel to the same
model bit for bit."""
import ctypes as C
import gc
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib, layouts
from multigrid_amd.constants import Color, Type
from tests.test_action_mask import MaskOracle
from tests.test_env_snapshot import make_env
from tests.test_episode_stats import actions_for
from tests.test_state_key import _i64, cell_bytes_of, triples_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
EMPTY, WALL, FLOOR, DOOR, KEY, BALL, BOX, GOAL, LAVA = 1, 2, 3, 4, 5, 6, 7, 8, 9
OPEN, CLOSED, LOCKED = 0, 1, 2
THROUGH_CLOSED, THROUGH_LOCKED, THROUGH_OBJECTS, AVOID_LAVA = 1, 2, 4, 8       # MGX_DIST_*
LEFT, RIGHT, FORWARD, DONE = 0, 1, 2, 6


# ---- the rule, in NumPy ------------------------------------------------------------------------------------------------------------

def model_passable(t, st, flags):
    door = t == DOOR
    return (np.isin(t, (EMPTY, FLOOR, GOAL)) | ((t == LAVA) & (not flags & AVOID_LAVA)) | (door & (st == OPEN))
            | (door & (st == CLOSED) & bool(flags & THROUGH_CLOSED)) | (door & (st == LOCKED) & bool(flags & THROUGH_LOCKED))
            | (np.isin(t, (KEY, BALL, BOX)) & bool(flags & THROUGH_OBJECTS)))


def model_sources(cb, cells, agents, spec, type_mask=0, colour_mask=0xFF, agent_mask=0, points=None):
    """(sources, t, st): bool[n,H,W] and the cells' types and states"""
    tri = triples_of(cb, cells).astype(np.int64)
    n, W, H = tri.shape[0], spec.width, spec.height
    t, col, st = ((tri[..., k] & m).reshape(n, H, W) for k, m in enumerate((15, 7, 3)))
    src = (((type_mask >> t) & 1) & ((colour_mask >> col) & 1)).astype(bool)
    ag = np.asarray(agents).astype(np.int64)
    rows = np.arange(n)
    for a in range(ag.shape[1]):
        if (agent_mask >> a) & 1:
            x, y = ag[:, a, 2], ag[:, a, 3]
            ok = (x < W) & (y < H)
            src[rows[ok], y[ok], x[ok]] = True
    if points is not None:
        pts = np.asarray(points).astype(np.int64)
        for k in range(pts.shape[1]):
            x, y = pts[:, k, 0], pts[:, k, 1]
            ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            src[rows[ok], y[ok], x[ok]] = True
    return src, t, st


def model_distance(cb, cells, agents, spec, *, type_mask=0, colour_mask=0xFF, agent_mask=0, points=None, flags=0):
    """(field i16[n,H,W], agent_dist i16[n,A]) of n rows: cells [n,...] in the format `cb`, agents u8[n,A,8], points i16[n,P,2] or
    None -- level k + 1 is the dilation of level k by the four neighbours, cut to the passable cells no earlier level holds"""
    src, t, st = model_sources(cb, cells, agents, spec, type_mask, colour_mask, agent_mask, points)
    passable = model_passable(t, st, flags)
    n, H, W = src.shape
    d = np.full((n, H, W), -1, np.int16)
    d[src] = 0
    seen, front, k = src.copy(), src, 0
    while front.any():
        k += 1
        nb = np.zeros_like(front)
        nb[:, 1:] |= front[:, :-1]
        nb[:, :-1] |= front[:, 1:]
        nb[:, :, 1:] |= front[:, :, :-1]
        nb[:, :, :-1] |= front[:, :, 1:]
        front = nb & passable & ~seen
        d[front] = k
        seen |= front
    assert k <= H * W
    ag = np.asarray(agents).astype(np.int64)
    x, y = ag[..., 2], ag[..., 3]
    inside = (x < W) & (y < H)
    ad = np.where(inside, d[np.arange(n)[:, None], np.where(inside, y, 0), np.where(inside, x, 0)], -1).astype(np.int16)
    return d, ad


def agents_at(positions, n=1):
    """u8[n,A,8] agent rows at the (x, y) positions, carrying nothing"""
    ag = np.zeros((n, len(positions), 8), np.uint8)
    ag[..., 5] = EMPTY
    for a, (x, y) in enumerate(positions):
        ag[:, a, 2:4] = (x, y)
    return ag


def test_the_model_on_a_worked_example():
    """      x 0 1 2 3 4          to the key at (3, 1), through the closed door at (2, 1):
        y 0  # # # # #              # # # # #
          1  # . D K #              # 2 1 0 #        the agent at (1, 3) walks up (1, 2), (1, 1), through the door, onto the key
          2  # . # . #              # 3 # 1 #
          3  # . # L #              # 4 # 2 #        (3, 3) is lava: passable unless avoided
          4  # # # # #              # # # # #
    without through={"closed"} the left column is cut off: the door stops the flood, being no source itself"""
    spec = EnvSpec(5, 5, 2, 3)
    g, _ = layouts.empty_layout(5, 1)
    g[1:4, 1:4] = (EMPTY, 0, 0)
    g[2:4, 2] = (WALL, 5, 0)
    g[1, 2] = (DOOR, 4, CLOSED)
    g[1, 3] = (KEY, 4, 0)
    g[3, 3] = (LAVA, 0, 0)
    ag = agents_at([(1, 3), (3, 3)])
    key = dict(type_mask=1 << KEY)
    d, ad = model_distance(3, g[None], ag, spec, **key)
    assert d[0].tolist() == [[-1] * 5, [-1, -1, -1, 0, -1], [-1, -1, -1, 1, -1], [-1, -1, -1, 2, -1], [-1] * 5] and ad.tolist() == [[-1, 2]]
    d, ad = model_distance(3, g[None], ag, spec, flags=THROUGH_CLOSED, **key)
    assert d[0].tolist() == [[-1] * 5, [-1, 2, 1, 0, -1], [-1, 3, -1, 1, -1], [-1, 4, -1, 2, -1], [-1] * 5] and ad.tolist() == [[4, 2]]
    d, ad = model_distance(3, g[None], ag, spec, flags=THROUGH_CLOSED | AVOID_LAVA, **key)
    assert d[0, 3].tolist() == [-1, 4, -1, -1, -1] and ad.tolist() == [[4, -1]]
    assert model_distance(3, g[None], ag, spec, flags=THROUGH_LOCKED, **key)[1].tolist() == [[-1, 2]]      # closed is not locked
    assert model_distance(3, g[None], ag, spec, colour_mask=1 << 3, **key)[0].max() == -1                   # no purple key: no source
    # the other selectors: agent 0's own cell, and a point (one outside the grid is ignored); a key is walked over with "objects"
    d, ad = model_distance(3, g[None], ag, spec, agent_mask=1, flags=THROUGH_CLOSED | THROUGH_OBJECTS)
    assert ad.tolist() == [[0, 6]] and d[0, 1].tolist() == [-1, 2, 3, 4, -1]
    pts = np.array([[[3, 2], [5, 1], [-1, 0]]], np.int16)
    assert model_distance(3, g[None], ag, spec, points=pts)[0][0, :, 3].tolist() == [-1, -1, 0, 1, -1]      # the key stops the flood


# ---- random grids ------------------------------------------------------------------------------------------------------------------

def random_grids(r, n, W, H, A, cb, wall=0.3):
    """n random grids as the model, the host program and the kernel take them -- walls at density `wall`, doors of all three states,
    keys, balls, boxes (with contents where the format holds them), lava, goals, floor -- in the format cb, and agents anywhere in the
    grid, a part of them terminated.  {"cells", "agents"}"""
    other = [(DOOR, OPEN), (DOOR, CLOSED), (DOOR, LOCKED), (KEY, 0), (BALL, 0), (BOX, 0), (GOAL, 0), (LAVA, 0), (FLOOR, 0), (0, 0)]
    pal = np.array([(EMPTY, 0)] + [(WALL, 0)] + other, np.uint8)
    p = np.array([1.0 - wall - 0.2, wall] + [0.2 / len(other)] * len(other))
    pick = pal[r.choice(len(pal), size=(n, H, W), p=p)]
    g = np.zeros((n, H, W, 3), np.uint8)
    g[..., 0], g[..., 2] = pick[..., 0], pick[..., 1]
    g[..., 1] = r.integers(0, 6, size=(n, H, W))
    if cb != 1:                                                              # what a box holds is never looked at
        box = g[..., 0] == BOX
        g[..., 2] = np.where(box & (r.random((n, H, W)) < 0.5), r.integers(1, 8, size=(n, H, W)) << 2 | r.integers(0, 6, size=(n, H, W)) << 5, g[..., 2])
    cells = g if cb == 3 else (layouts.pack_cells8(g) if cb == 1 else layouts.pack_cells(g))
    ag = np.zeros((n, A, 8), np.uint8)
    ag[..., 0] = r.integers(0, 6, size=(n, A))
    ag[..., 1] = r.integers(0, 4, size=(n, A))
    ag[..., 2] = r.integers(0, W, size=(n, A))
    ag[..., 3] = r.integers(0, H, size=(n, A))
    ag[..., 4] = r.random((n, A)) < 0.15
    ag[..., 5] = EMPTY
    return {"cells": np.ascontiguousarray(cells), "agents": ag}


def random_query(r, n, W, H, A, P=2):
    """a query with every selector in play: one or two types (any colour, or three of them), some agents, P points per row -- one in
    five outside the grid -- and any flags"""
    q = dict(type_mask=int(sum({1 << int(t) for t in r.choice([GOAL, KEY, DOOR, BALL, WALL, LAVA], size=int(r.integers(1, 3)))})),
             colour_mask=0xFF if r.random() < 0.5 else int(sum({1 << int(c) for c in r.integers(0, 6, size=3)})),
             agent_mask=int(r.integers(0, 1 << min(A, 3))), flags=int(r.integers(0, 16)))
    pts = np.stack((r.integers(0, W, size=(n, P)), r.integers(0, H, size=(n, P))), axis=-1)
    out = r.random((n, P)) < 0.2
    pts[out] = np.array([(-1, 0), (0, -3), (W, 0), (1, H), (300, 300), (-32768, 32767)])[r.integers(0, 6, size=int(out.sum()))]
    q["points"] = np.ascontiguousarray(pts.astype(np.int16))
    return q


def spec_for(W, H, A, cb=2):
    return EnvSpec(W, H, A, 3, cell_bytes=cb)


# ---- csrc/mgx_distance.h, built by g++ into a program of its own -------------------------------------------------------------------

HOST_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mgx_distance.h"
#include "mgx_aux_geom.h"
using namespace mgx;
static long long rd(FILE *f) { long long v = 0; if (fread(&v, 8, 1, f) != 1) return -1; return v; }
static std::vector<uint8_t> bytes(FILE *f, size_t n) {
    std::vector<uint8_t> b(n);
    if (n && fread(b.data(), 1, n, f) != n) { printf("short input\n"); exit(2); }
    return b;
}
// Every (type, colour, state) a cell can show, with and without overlap: base passability is the forward bit of an empty-handed agent
// in front of that cell with nobody there; and each flag moves exactly the cells the header names.
static long long exhaustive() {
    long long checked = 0;
    for (uint32_t t = 0; t < 16; ++t)
        for (uint32_t c = 0; c < 8; ++c)
            for (uint32_t s = 0; s < 4; ++s)
                for (int overlap = 0; overlap < 2; ++overlap) {
                    const uint32_t cell = t | c << 8 | s << 16;
                    const bool fwd = (mask_front_bits(cell, CELL_EMPTY, false, overlap != 0, false, false) & MASK_FORWARD) != 0;
                    if (dist_passable(cell, 0) != fwd) { printf("FAILED type %u colour %u state %u: forward %d\n", t, c, s, (int)fwd); return -1; }
                    for (uint32_t flags = 0; flags < 16; ++flags) {
                        bool want = fwd;
                        if ((flags & MGX_DIST_AVOID_LAVA) && t == (uint32_t)T_LAVA) want = false;
                        if ((flags & MGX_DIST_THROUGH_CLOSED) && t == (uint32_t)T_DOOR && s == (uint32_t)S_CLOSED) want = true;
                        if ((flags & MGX_DIST_THROUGH_LOCKED) && t == (uint32_t)T_DOOR && s == (uint32_t)S_LOCKED) want = true;
                        if ((flags & MGX_DIST_THROUGH_OBJECTS) && (t == (uint32_t)T_KEY || t == (uint32_t)T_BALL || t == (uint32_t)T_BOX)) want = true;
                        if (dist_passable(cell, flags) != want) { printf("FAILED type %u state %u flags %u\n", t, s, flags); return -1; }
                        ++checked;
                    }
                }
    return checked;
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    for (long long kind; (kind = rd(f)) >= 0;) {
        if (kind == 0) {                                   // grids: W H A cb n type_mask colour_mask agent_mask flags P, then cells, agents, points
            const int W = (int)rd(f), H = (int)rd(f), A = (int)rd(f), cb = (int)rd(f), n = (int)rd(f);
            MgxDistance q;
            memset(&q, 0, sizeof q);
            q.type_mask = (uint32_t)rd(f); q.colour_mask = (uint32_t)rd(f); q.agent_mask = (uint32_t)rd(f); q.flags = (uint32_t)rd(f);
            q.num_points = (int)rd(f);
            const size_t HW = (size_t)W * H, tile = HW * cb;
            const auto cells = bytes(f, tile * n), agents = bytes(f, (size_t)n * A * 8), pts = bytes(f, (size_t)n * q.num_points * 4);
            for (int i = 0; i < n; ++i) {
                std::vector<uint16_t> store((tile + 1) / 2);                                 // (their own allocations: an over-read shows;
                memcpy(store.data(), cells.data() + i * tile, tile);                         //  2-byte aligned for the 16-bit cells)
                const uint8_t *tile_i = reinterpret_cast<const uint8_t *>(store.data());
                std::vector<uint32_t> dec(HW);
                for (size_t p = 0; p < HW; ++p) dec[p] = mask_cell(cb, tile_i + p * cb);
                std::vector<uint8_t> ag(agents.begin() + (size_t)i * A * 8, agents.begin() + (size_t)(i + 1) * A * 8);
                std::vector<int16_t> pt((size_t)q.num_points * 2), field(HW, 77), ad(A, 77), d(HW);
                if (q.num_points) memcpy(pt.data(), pts.data() + (size_t)i * q.num_points * 4, (size_t)q.num_points * 4);
                std::vector<int32_t> queue(HW);
                dist_reference(W, H, A, dec.data(), ag.data(), q, q.num_points ? pt.data() : nullptr, field.data(), ad.data(), d.data(), queue.data());
                for (size_t p = 0; p < HW; ++p) printf("%d ", (int)field[p]);
                printf("|");
                for (int a = 0; a < A; ++a) printf(" %d", (int)ad[a]);
                printf("\n");
            }
        } else if (kind == 1) {                            // the exhaustive table
            const long long c = exhaustive();
            if (c < 0) return 1;
            printf("exhaustive %lld\n", c);
        } else {                                           // geometry: W H n
            const int W = (int)rd(f), H = (int)rd(f);
            const long long n = rd(f);
            const DistanceGeom g = distance_geom(W, H, n);
            if (g.group < H || g.group < 4 || (g.group & (g.group - 1)) || (g.group > 4 && g.group / 2 >= H) || g.per * g.group != 64
                || g.wp < W || (g.wp & (g.wp - 1)) || (g.wp > 1 && g.wp / 2 >= W) || g.rpb * g.wp != 64
                || g.nwaves * g.per < n || (g.nwaves - 1) * g.per >= n || g.blocks * kDistWpb < g.nwaves
                || (g.blocks - 1) * kDistWpb >= g.nwaves) { printf("FAILED geometry\n"); return 1; }
            printf("%d %d %d %d %lld %lld\n", g.group, g.per, g.wp, g.rpb, (long long)g.nwaves, (long long)g.blocks);
        }
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no C++ compiler"
    d = tmp_path_factory.mktemp("distance_host")
    src = d / "distance_host.cpp"
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
        return [ln for ln in p.stdout.split("\n") if ln]
    return run


def grids_payload(spec, cb, rows, q):
    n = rows["agents"].shape[0]
    pts = q.get("points")
    head = _i64(0, spec.width, spec.height, spec.num_agents, cb, n, q.get("type_mask", 0), q.get("colour_mask", 0xFF), q.get("agent_mask", 0),
                q.get("flags", 0), 0 if pts is None else pts.shape[1])
    return head + rows["cells"].tobytes() + rows["agents"].tobytes() + (b"" if pts is None else pts.tobytes())


def field_lines(d, ad):
    """what the host program prints for (field, agent_dist)"""
    return ["".join(f"{int(v)} " for v in f.reshape(-1)) + "|" + "".join(f" {int(v)}" for v in a) for f, a in zip(d, ad)]


HOST_SHAPES = ((3, 3), (4, 5), (6, 7), (16, 16), (64, 9))


@pytest.fixture(scope="module")
def host_cases():
    r = np.random.default_rng(33)
    payload, want, fields = [], [], []
    for W, H in HOST_SHAPES:
        for A in (1, 4):
            for cb in (2, 1, 3):
                for _ in range(3):
                    spec = spec_for(W, H, A, cb)
                    rows = random_grids(r, 6, W, H, A, cb)
                    q = random_query(r, 6, W, H, A)
                    d, ad = model_distance(cb, rows["cells"], rows["agents"], spec, **q)
                    payload.append(grids_payload(spec, cb, rows, q))
                    want += field_lines(d, ad)
                    fields.append(d.reshape(-1))
    return b"".join(payload), want, np.concatenate(fields)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_header_gives_the_models_fields(host_programs, host_cases, which):
    payload, want, fields = host_cases
    got = host_programs(which, payload)
    assert len(got) == len(want) == len(HOST_SHAPES) * 2 * 3 * 3 * 6
    assert got == want
    assert (fields == -1).sum() > 1000 and (fields == 0).sum() > 1000 and (fields > 5).sum() > 100      # not hollow


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_base_passability_is_the_forward_bit_on_every_cell(host_programs, which):
    """the table runs inside the program (HOST_MAIN: exhaustive): 16 types x 8 colours x 4 states x overlap or not, each against
    mask_front_bits' forward bit with nobody present, and then under each of the 16 flag sets"""
    assert host_programs(which, _i64(1)) == [f"exhaustive {16 * 8 * 4 * 2 * 16}"]


def test_the_worked_example_through_the_header(host_programs):
    spec = EnvSpec(5, 5, 2, 3)
    g, _ = layouts.empty_layout(5, 1)
    g[1:4, 1:4] = (EMPTY, 0, 0)
    g[2:4, 2] = (WALL, 5, 0)
    g[1, 2], g[1, 3], g[3, 3] = (DOOR, 4, CLOSED), (KEY, 4, 0), (LAVA, 0, 0)
    rows = {"cells": g[None].copy(), "agents": agents_at([(1, 3), (3, 3)])}
    for flags in (0, THROUGH_CLOSED, THROUGH_CLOSED | AVOID_LAVA):
        q = dict(type_mask=1 << KEY, flags=flags)
        assert host_programs("sanitized", grids_payload(spec, 3, rows, q)) == field_lines(*model_distance(3, rows["cells"], rows["agents"], spec, **q))


def geometry(W, H, n):
    """(group, per, wp, rpb, wavefronts, workgroups) of a mgx_distance launch: csrc/mgx_aux_geom.h restated (held to it below)"""
    group, wp = 4, 1
    while group < H:
        group *= 2
    while wp < W:
        wp *= 2
    per = 64 // group
    nwaves = (n + per - 1) // per
    return group, per, wp, 64 // wp, nwaves, (nwaves + 3) // 4


def test_the_launch_geometry_is_what_the_gpu_tests_name(host_programs):
    cases = [(W, H, n) for W, H in ((1, 1), (3, 3), (4, 5), (6, 7), (8, 8), (16, 16), (9, 17), (64, 33), (3, 64), (64, 64), (33, 32))
             for n in (1, 2, 15, 16, 17, 65536, (1 << 31) + 1)]
    got = host_programs("sanitized", b"".join(_i64(2, *c) for c in cases))
    assert [tuple(int(v) for v in ln.split()) for ln in got] == [geometry(*c) for c in cases]
    assert [geometry(W, H, 70)[0] for W, H in ((3, 3), (4, 5), (8, 8), (9, 17), (64, 33))] == [4, 8, 8, 32, 64]


# ---- the engine tie: the oracle walks down the field -------------------------------------------------------------------------------

def _descent_class(ci, B=12):
    """(spec, start state): Empty 8x8 with a random start, or a LockedHallway of 2 x 2 rooms whose doors stand open and whose last
    empty cell holds a goal.  One agent: nobody is ever in the way."""
    grids, agents, auxs = [], [], []
    for s in range(B):
        lr, nr = np.random.default_rng(2000 * ci + s), np.random.default_rng(7000 * ci + s)
        if ci == 0:
            spec = EnvSpec(8, 8, 1, 3, max_steps=400)
            g, a = layouts.empty_layout(8, 1, None, None, lr)
            aux = np.zeros(16, np.uint8)
        else:
            spec = EnvSpec(13, 9, 1, 3, max_steps=400, env_kind="lockedhallway")
            g, a = layouts.lockedhallway_layout(4, 5, 1, 2, 1, lr, nr)
            g[g[..., 0] == DOOR, 2] = OPEN
            aux = layouts.make_aux("lockedhallway", g)
            free = np.argwhere(g[..., 0] == EMPTY)
            y, x = free[lr.integers(0, len(free))]
            g[y, x] = (GOAL, 1, 0)
        grids.append(g); agents.append(a); auxs.append(aux)
    rng = np.random.default_rng(41 + ci).integers(0, 2 ** 63, size=(B, 4), dtype=np.int64).astype(np.uint64)
    rng[:, 2] |= np.uint64(1)
    return spec, dict(grid=np.ascontiguousarray(np.stack(grids)), agents=np.ascontiguousarray(np.stack(agents)), rng=rng,
                      step_count=np.zeros(B, np.int32), aux=np.ascontiguousarray(np.stack(auxs)))


def _queue_flood(passable, sources):
    """an independent shortest-path count for one grid: a plain queue, cell after cell"""
    H, W = passable.shape
    d = np.full((H, W), -1, np.int64)
    todo = [(int(y), int(x)) for y, x in np.argwhere(sources)]
    for y, x in todo:
        d[y, x] = 0
    while todo:
        y, x = todo.pop(0)
        for ny, nx in ((y, x + 1), (y, x - 1), (y + 1, x), (y - 1, x)):
            if 0 <= ny < H and 0 <= nx < W and d[ny, nx] < 0 and passable[ny, nx]:
                d[ny, nx] = d[y, x] + 1
                todo.append((ny, nx))
    return d


@pytest.mark.parametrize("ci", [0, 1])
def test_the_oracle_reaches_a_goal_in_agent_dist_forward_moves(ci):
    from oracle import binding as ob
    spec, st = _descent_class(ci)
    B, W, H = st["agents"].shape[0], spec.width, spec.height
    field, ad = model_distance(3, st["grid"], st["agents"], spec, type_mask=1 << GOAL)
    reach = ad[:, 0] >= 0                                                    # (a key in a doorway can cut a goal off: that env stays put)
    assert (ad[:, 0] != 0).all() and reach.sum() >= B - 2 and len(set(ad[:, 0].tolist())) > 3
    for b in range(B):                                                       # there is no shorter way
        t, s = st["grid"][b, ..., 0], st["grid"][b, ..., 2]
        assert (_queue_flood(model_passable(t, s & 3, 0), t == GOAL) == field[b]).all()
    moves, turns = np.zeros(B, np.int64), 0
    for _ in range(4 * int(ad.max()) + 4):
        x, y, d = (st["agents"][:, 0, k].astype(np.int64) for k in (2, 3, 1))
        here = field[np.arange(B), y, x]
        acts = np.full((B, 1), DONE, np.int8)
        expect = {}
        for b in np.flatnonzero(here > 0):
            want = [k for k, (dx, dy) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))) if field[b, y[b] + dy, x[b] + dx] == here[b] - 1]
            assert want, "a cell of level k > 0 has a neighbour of level k - 1"
            if d[b] in want:
                acts[b, 0], expect[b] = FORWARD, d[b]
            else:
                acts[b, 0] = LEFT if (d[b] - 1) % 4 in want else RIGHT
                turns += 1
        if not (here > 0).any():
            break
        ob.step_batch(spec.as_dict(), st["grid"], st["agents"], st["rng"], st["step_count"], acts, st["aux"])
        for b, dd in expect.items():                                         # every forward succeeded: one level down
            dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[dd]
            assert (int(st["agents"][b, 0, 2]), int(st["agents"][b, 0, 3])) == (x[b] + dx, y[b] + dy)
            moves[b] += 1
    x, y = st["agents"][:, 0, 2].astype(np.int64), st["agents"][:, 0, 3].astype(np.int64)
    assert (field[np.arange(B), y, x][reach] == 0).all() and (st["grid"][np.arange(B), y, x, 0][reach] == GOAL).all()
    assert moves[reach].tolist() == ad[reach, 0].tolist() and (moves[~reach] == 0).all() and turns > 0     # exactly k forwards; turns were free


# ---- the Python layer over the model -----------------------------------------------------------------------------------------------

class DistOracle(MaskOracle):
    """the oracle launcher + env_copy + action_mask (tests/test_action_mask.py) + distance, which is the model above and refuses what
    mgx_distance refuses; `dist_calls` records (n, members, query without its points, which outputs)."""

    def __init__(self, spec):
        super().__init__(spec)
        self.dist_calls = []

    def distance(self, n, rows, n_rows, idx, query, field, agent_dist, bad):
        pts = query.get("points")
        self.dist_calls.append((n, sorted(k for k, v in rows.items() if v is not None), {k: v for k, v in query.items() if k != "points"},
                                None if pts is None else tuple(pts.shape), field is not None, agent_dist is not None))
        sp = self.spec
        assert (field is None) != (agent_dist is None)
        if sp.width > 64 or sp.height > 64:
            raise _lib.MgxError(_lib.ERR_UNSUPPORTED, "mgx_distance")
        r = self._np(rows)
        for out, shape in ((field, (n, sp.height, sp.width)), (agent_dist, (n, sp.num_agents))):
            assert out is None or (tuple(out.shape) == shape and out.dtype is torch.int16)
        for i in range(n):
            s = i if idx is None else int(idx[i])
            if not 0 <= s < n_rows:
                if bad is not None:
                    bad[0] += 1
                    bad[1] = min(int(bad[1]), min(i, INT32_MAX))
                continue
            q = {k: v for k, v in query.items() if k != "points"}
            d, ad = model_distance(cell_bytes_of(sp), r["cells"][s:s + 1], r["agents"][s:s + 1], sp,
                                   points=None if pts is None else pts[i:i + 1].numpy(), **q)
            if field is not None:
                field[i] = torch.from_numpy(d[0])
            else:
                agent_dist[i] = torch.from_numpy(ad[0])


SPEC = EnvSpec(5, 5, 2, 3, max_steps=6, allow_agent_overlap=False)


def env_fields(env, ids=None, **q):
    """the model on what the env shows: .grid (byte triples) and the agent rows"""
    g, a = env.grid.cpu().numpy(), env.agents.cpu().numpy()
    ids = np.arange(g.shape[0]) if ids is None else np.asarray(ids)
    return model_distance(3, g[ids], a[ids], env.spec, **q)


def stepped_env(B=7, backend=None):
    env = make_env("pool", B=B, spec=SPEC, backend=backend or DistOracle(SPEC))
    for a in actions_for(B, 2, 3, 4):
        env.step(a, auto_reset=True)
    return env


def test_distance_of_a_batch_and_its_arguments():
    B, A, H, W = 7, 2, 5, 5
    env = stepped_env(B)
    be = env.backend
    field = env.distance_field(types=[Type.goal])
    assert field.dtype is torch.int16 and tuple(field.shape) == (B, H, W) and field.device == env.device
    want_f, want_a = env_fields(env, type_mask=1 << GOAL)
    assert field.numpy().tolist() == want_f.tolist() and (want_f >= 0).sum() == B * 9 and want_f.max() == 4
    assert be.dist_calls[-1] == (B, ["agents", "cells"], dict(type_mask=1 << GOAL, colour_mask=0xFF, agent_mask=0, flags=0), None, True, False)
    dist = env.agent_distance(types=[8])
    assert dist.dtype is torch.int16 and tuple(dist.shape) == (B, A) and dist.numpy().tolist() == want_a.tolist()
    assert len(np.unique(want_a)) > 1 and be.dist_calls[-1][4:] == (False, True)
    # every selector and flag reaches the launcher as the header's bits
    pts = torch.tensor([[[1, 1], [9, 9]]] * B, dtype=torch.int16)
    env.distance_field(types=(Type.goal, Type.key), colors=[Color.green, 0], agents=[1], points=pts, through={"closed", "objects"}, avoid_lava=True)
    assert be.dist_calls[-1][2:4] == (dict(type_mask=1 << 8 | 1 << 5, colour_mask=3, agent_mask=2, flags=1 | 4 | 8), (B, 2, 2))
    env.agent_distance(agents=range(2), through="locked")
    assert be.dist_calls[-1][2] == dict(type_mask=0, colour_mask=0xFF, agent_mask=3, flags=2)
    got = env.distance_field(points=pts)
    assert got.numpy().tolist() == env_fields(env, points=pts.numpy())[0].tolist() and (got[:, 1, 1] == 0).all()
    assert env.agent_distance(agents=[0])[:, 0].tolist() == [0] * B
    # chosen envs, repeats allowed; out= is written and handed back; points go by OUTPUT row
    ids = torch.tensor([6, 0, 0, 3])
    out = torch.full((4, H, W), 77, dtype=torch.int16)
    assert env.distance_field(ids, types=[Type.goal], out=out) is out and out.tolist() == field[ids].tolist()
    out = torch.full((4, A), 77, dtype=torch.int16)
    assert env.agent_distance(ids, types=[Type.goal], out=out) is out and out.tolist() == dist[ids].tolist()
    p4 = torch.tensor([[[1, 1]], [[2, 2]], [[3, 3]], [[1, 3]]], dtype=torch.int16)
    got = env.distance_field(ids, points=p4)
    assert got.numpy().tolist() == env_fields(env, ids.numpy(), points=p4.numpy())[0].tolist()
    assert [int(got[k, y, x]) for k, (x, y) in enumerate(((1, 1), (2, 2), (3, 3), (1, 3)))] == [0] * 4 and int(got[1, 1, 1]) == 2
    assert env.agent_distance(torch.zeros(0, dtype=torch.int64), types=[8]).shape == (0, A)
    # refusals
    for kw, msg in ((dict(), "names no source"), (dict(colors=[1]), "pass types= with it"), (dict(types=[]), "names no source"),
                    (dict(types=[8], through=["open"]), "through= holds 'open'"), (dict(agents=[2]), r"agent index must lie in \[0, 2\)"),
                    (dict(agents=[-1]), "agent index"), (dict(types=[16]), "a Type or an int"), (dict(types=[8], colors=[8]), "a Color or an int"),
                    (dict(types="goal"), "types must be an iterable of ints"), (dict(types=8), "types must be an iterable of ints"),
                    (dict(points=torch.zeros((B, 2), dtype=torch.int16)), "points must be a contiguous int16 tensor"),
                    (dict(points=torch.zeros((B, 1, 2), dtype=torch.int32)), "points must be a contiguous int16 tensor"),
                    (dict(points=torch.zeros((B + 1, 1, 2), dtype=torch.int16)), "points must be a contiguous int16 tensor"),
                    (dict(points=torch.zeros((B, 1, 4), dtype=torch.int16)[..., ::2]), "points must be a contiguous int16 tensor"),
                    (dict(points=torch.zeros((B, 0, 2), dtype=torch.int16)), "names no source")):
        for method in (env.distance_field, env.agent_distance):
            with pytest.raises(ValueError, match=msg):
                method(**kw)
    for t in (torch.arange(4, dtype=torch.int32), torch.arange(4).reshape(2, 2), torch.arange(8)[::2], [0, 1]):
        with pytest.raises(ValueError, match="env_ids must be a contiguous int64 tensor"):
            env.distance_field(t, types=[8])
    for bad_out in (torch.zeros((B, H, W), dtype=torch.int32), torch.zeros((B + 1, H, W), dtype=torch.int16), torch.zeros((B, A), dtype=torch.int16),
                    torch.zeros((B, H, 2 * W), dtype=torch.int16)[..., ::2], np.zeros((B, H, W), np.int16)):
        with pytest.raises(ValueError, match="out= must be a contiguous int16 tensor of shape"):
            env.distance_field(types=[8], out=bad_out)
    for bad_out in (torch.zeros((B, A), dtype=torch.uint8), torch.zeros((B, H, W), dtype=torch.int16), torch.zeros((4, A), dtype=torch.int16)):
        with pytest.raises(ValueError, match="out= must be a contiguous int16 tensor of shape"):
            env.agent_distance(types=[8], out=bad_out)
    env._session = object()
    with pytest.raises(RuntimeError, match="persistent session"):
        env.distance_field(types=[8])
    env._session = None
    with pytest.raises(RuntimeError, match="no state loaded"):
        BatchedMultiGridEnv(SPEC, B, "cpu", backend=DistOracle(SPEC)).agent_distance(types=[8])
    with pytest.raises(RuntimeError, match="sub-shard of split"):
        env.split(2)[0].distance_field(types=[8])
    # ids out of range: their rows are left alone, and check_errors() tells -- in the words it has for snapshots
    out = torch.full((4, A), 77, dtype=torch.int16)
    env.agent_distance(torch.tensor([1, B, -1, 2]), types=[8], out=out)
    assert out.tolist() == [dist[1].tolist(), [77] * A, [77] * A, dist[2].tolist()]
    with pytest.raises(ValueError, match=r"2 pair\(s\) named an env id or a snapshot row out of range.*first at pair 1"):
        env.check_errors()
    env.check_errors()
    assert env.distance_field(torch.tensor([B]), types=[8]).tolist() == [[[-1] * W] * H]     # (a fresh output: no way anywhere)
    with pytest.raises(ValueError, match="out of range"):
        env.check_errors()


def test_a_snapshots_rows_have_the_distances_of_their_moment():
    B, A = 40, 2
    env = stepped_env(B)
    snap = env.snapshot()
    q = dict(agents=[1], types=[Type.goal])
    at_snap, field_at_snap = env.agent_distance(**q), env.distance_field(**q)
    for a in actions_for(B, A, 2, 9):
        env.step(a, auto_reset=True)
    assert (env.agent_distance(**q) != at_snap).any()
    assert snap.agent_distance(**q).tolist() == at_snap.tolist() and snap.distance_field(**q).tolist() == field_at_snap.tolist()
    assert env.backend.dist_calls[-1][:2] == (B, ["agents", "cells"])
    rows = torch.tensor([3, 3, 39])
    out = torch.zeros((3, 5, 5), dtype=torch.int16)
    assert snap.distance_field(rows, out=out, **q) is out and out.tolist() == field_at_snap[rows].tolist()
    out = torch.zeros((3, A), dtype=torch.int16)
    assert snap.agent_distance(rows, out=out, **q) is out and out.tolist() == at_snap[rows].tolist()
    env.restore(snap)
    assert env.agent_distance(**q).tolist() == at_snap.tolist()
    # a snapshot row out of range is reported by the env that took the snapshot
    snap.agent_distance(torch.tensor([0, B]), **q)
    with pytest.raises(ValueError, match=r"1 pair\(s\) named an env id or a snapshot row out of range.*first at pair 1"):
        env.check_errors()
    with pytest.raises(ValueError, match="rows must be a contiguous int64 tensor"):
        snap.distance_field(torch.arange(3, dtype=torch.int32), **q)
    with pytest.raises(ValueError, match="out= must be a contiguous int16 tensor of shape"):
        snap.agent_distance(rows, out=torch.zeros((B, A), dtype=torch.int16), **q)
    with pytest.raises(ValueError, match="names no source"):
        snap.distance_field()
    with pytest.raises(ValueError, match=r"points must be a contiguous int16 tensor of shape \(3, P, 2\)"):
        snap.distance_field(rows, points=torch.zeros((B, 1, 2), dtype=torch.int16))
    del env
    gc.collect()
    with pytest.raises(RuntimeError, match="the env this snapshot was taken from is gone"):
        snap.distance_field(**q)


def test_the_layout_marker_stays_armed_across_a_distance_query():
    B = 7
    env = make_env("pool", B=B, spec=SPEC, backend=DistOracle(SPEC), pool_size=1)
    assert env._tracks() and env._mark["armed"] and env._marker.tolist() == [0] * B
    before = {k: getattr(env, k).clone() for k in ("_marker", "rng", "step_count", "episode", "aux")}
    env.distance_field(types=[8])
    env.agent_distance(torch.tensor([1, 2]), agents=[0])
    assert env._mark["armed"] and all((getattr(env, k) == v).all() for k, v in before.items())


def test_a_side_above_64_is_refused_as_unsupported():
    spec = EnvSpec(65, 5, 1, 3, max_steps=6)
    env = BatchedMultiGridEnv(spec, 2, "cpu", backend=DistOracle(spec))
    g = np.zeros((5, 65, 3), np.uint8)
    g[...] = (WALL, 5, 0)
    g[1:4, 1:64] = (EMPTY, 0, 0)
    env.load_state(g, agents_at([(1, 1)])[0])
    for method in (env.distance_field, env.agent_distance, env.snapshot().distance_field):
        with pytest.raises(_lib.MgxError, match="mgx_distance") as e:
            method(agents=[0])
        assert e.value.code == _lib.ERR_UNSUPPORTED


def test_the_example_finds_the_goal_with_fewer_expansions_than_breadth_first():
    """examples/best_first.py on 1024 envs of C2 (Empty-16x16), one root, a beam of 8, through an oracle launcher: both searches end
    at the same depth -- the heuristic never overestimates --, the informed one after a fraction of the expansions"""
    import importlib.util
    from multigrid_amd import workloads
    from tests.test_state_key import KeyOracle

    class SearchOracle(DistOracle, KeyOracle):
        pass
    mod_spec = importlib.util.spec_from_file_location("best_first", os.path.join(ROOT, "examples", "best_first.py"))
    mod = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(mod)
    out = mod.run("c2", roots=1, beam=8, depth=40, batch=1024, device="cpu", backend=SearchOracle(workloads.spec_of("c2")))
    best, breadth = out["best_first"], out["breadth_first"]
    assert best["found"] and breadth["found"] and best["depth"] == breadth["depth"] == 27      # 13 + 13 moves and one turn
    assert best["nodes_expanded"] * 3 < breadth["nodes_expanded"]
    with pytest.raises(ValueError, match="no goal cell"):
        mod.run("c3", batch=64, device="cpu", backend=SearchOracle(workloads.spec_of("c3")))


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------------

def test_c_abi_argument_validation():
    """what mgx_distance checks of its own, the return codes in the header's order; no call gets as far as a launch.  The checks of
    every row query: tests/test_row_query_abi.py"""
    from tests.test_row_query_abi import INV, UNS, P as p, dist_query as query, full, ref
    L = _lib.lib()
    sc = EnvSpec(65, 5, 2, 3, max_steps=4).to_c()         # (a side of 65: what is not refused as invalid is refused as unsupported)

    def D(sc_, n, src, idx=p, q=query(), field=p + 2, agent_dist=p + 6, bad=p):
        return L.mgx_distance(ref(sc_), n, ref(src), idx, ref(q), field, agent_dist, bad, None)
    a = full()
    assert D(sc, 4, a) == UNS and D(sc, 4, a, field=None) == UNS and D(sc, 4, a, agent_dist=None, idx=None, bad=None) == UNS
    tall = EnvSpec(5, 65, 2, 3).to_c()
    assert D(tall, 4, a) == UNS
    assert D(sc, 4, a, q=None) == INV
    for flags in (16, 17, 0x80000000):
        assert D(sc, 4, a, q=query(flags=flags)) == INV and D(sc, 0, a, q=query(flags=flags)) == INV
    assert D(sc, 4, a, q=query(num_points=-1)) == INV and D(sc, 0, a, q=query(num_points=-1)) == INV
    assert D(sc, 4, a, field=None, agent_dist=None) == INV
    assert D(sc, 4, a, q=query(points=None)) == INV and D(sc, 4, a, q=query(points=None, num_points=0)) == UNS
    bytes3 = EnvSpec(65, 5, 2, 3, cell_bytes=3).to_c()
    assert D(bytes3, 4, full(cells=p + 1)) == UNS                            # (byte triples: any alignment)
    assert D(sc, 4, a, field=p + 1) == INV
    assert D(sc, 4, a, agent_dist=p + 1) == INV and D(sc, 4, a, q=query(points=p + 1)) == INV


def test_the_export_is_the_headers_declaration():
    from tests.test_capi import declared_functions
    names = declared_functions()
    assert "mgx_distance" in names and "mgx_distance" in _lib.EXPORTS and getattr(_lib.lib(), "mgx_distance") is not None
    assert set(names) == set(_lib.EXPORTS) and _lib.lib().mgx_abi_version() == _lib.ABI_VERSION == 11
    assert (_lib.DIST_THROUGH_CLOSED, _lib.DIST_THROUGH_LOCKED, _lib.DIST_THROUGH_OBJECTS, _lib.DIST_AVOID_LAVA) == (1, 2, 4, 8)
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "DISTANCE FIELDS" in hdr and "MGX_DIST_THROUGH_CLOSED = 1, MGX_DIST_THROUGH_LOCKED = 2, MGX_DIST_THROUGH_OBJECTS = 4, MGX_DIST_AVOID_LAVA = 8" in hdr
    assert C.sizeof(_lib.MgxDistanceC) == 32 and _lib.MgxDistanceC.points.offset == 16 and _lib.MgxDistanceC.num_points.offset == 24
    from multigrid_amd import build
    assert os.path.join(build.CSRC, "mgx_distance.h") in build.DEPS and any(u[0] == "mgx_distance" for u in build.UNITS)
