"""Effective-action masks (include/mgx.h "ACTION MASKS", BatchedMultiGridEnv.action_mask, EnvSnapshot.action_mask) without a GPU.

`model_action_mask` states the rule in NumPy, from include/mgx.h alone, over the triples the library's own unpacking gives
(layouts.unpack_cells / unpack_cells8).  csrc/mgx_action_mask.h -- the statement the kernel is compiled from -- is built by g++ into a
stand-alone program, once plain and once under the address and undefined-behaviour sanitizers; it must give the model's masks on
random states of every cell format, and an exhaustive table in the same program holds it to `eval_agent` (csrc/mgx_rules.h), the
rule the kernels step by.  The two guarantees of the header -- sound, tight -- are checked against the CPU oracle on reachable
states.  The host logic of the two methods is driven through `MaskOracle`, the oracle launcher of tests/test_env_snapshot.py plus an
`action_mask` that IS the model.  tests/test_action_mask_gpu.py holds the kernel to the same model bit for bit.

The oracle walks: seeds 0..WALK_ENVS-1 per env class seed the layouts (np.random.default_rng(1000 * class index + seed)), the walk's
actions come from np.random.default_rng(77 + class index); with them the walks alone satisfy the census asserted below."""
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
from tests import hook_states
from tests.test_env_snapshot import CopyOracle, make_env
from tests.test_episode_stats import actions_for, empty_pool
from tests.test_state_key import _i64, cell_bytes_of, triples_of, valid_triples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
EXPAND = 1                                                                  # MGX_MASK_EXPAND
LEFT, RIGHT, FORWARD, PICKUP, DROP, TOGGLE, DONE = range(7)
EMPTY, WALL, FLOOR, DOOR, KEY, BALL, BOX, GOAL, LAVA = 1, 2, 3, 4, 5, 6, 7, 8, 9
OPEN, CLOSED, LOCKED = 0, 1, 2
KINDS = {"empty": 0, "blockedunlockpickup": 1, "redbluedoors": 2, "lockedhallway": 3, "rules": 4}


# ---- the rule, in NumPy ------------------------------------------------------------------------------------------------------------

def model_action_mask(cb, cells, agents, aux, spec):
    """masks u8[n,A] of n rows: cells [n,...] in the format `cb`, agents u8[n,A,8], aux u8[n,16] or None"""
    tri = triples_of(cb, cells).astype(np.int64)                            # what .grid shows: [n, H*W, 3]
    ag = np.asarray(agents).astype(np.int64)
    n, W, H = ag.shape[0], spec.width, spec.height
    d, x, y = ag[..., 1], ag[..., 2], ag[..., 3]
    live = ag[..., 4] == 0
    ctype, ccol = ag[..., 5], ag[..., 6]
    fx = x + (d == 0).astype(np.int64) - (d == 2).astype(np.int64)
    fy = y + (d == 1).astype(np.int64) - (d == 3).astype(np.int64)
    inside = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    c = tri[np.arange(n)[:, None], np.where(inside, fy * W + fx, 0)]         # (outside: a cell nobody looks at)
    t, col, st = c[..., 0] & 15, c[..., 1] & 7, c[..., 2] & 3
    present = ((x[:, None, :] == fx[:, :, None]) & (y[:, None, :] == fy[:, :, None])).any(-1)    # terminated rows count
    stale, hit = np.zeros_like(live), np.zeros_like(live)
    if aux is not None:
        ax = np.asarray(aux).astype(np.int64).reshape(n, 16)
        if spec.env_kind == "redbluedoors":
            stale = (ax[:, 4:5] != 0) & (fx == ax[:, 0:1]) & (fy == ax[:, 1:2])
        if spec.env_kind == "rules":
            for k in range(3):
                r = ax[:, 1 + 5 * k:6 + 5 * k]
                hit = hit | ((k < ax[:, 0:1]) & (r[:, 0:1] == 2) & (fx == r[:, 1:2]) & (fy == r[:, 2:3]))
    st = np.where(stale, CLOSED, st)                                        # that door's object state counts as closed
    door, nothing = t == DOOR, ctype == EMPTY
    overlap = np.isin(t, (EMPTY, GOAL, FLOOR, LAVA)) | (door & (st == OPEN))
    forward = overlap & (bool(spec.allow_agent_overlap) | ~present)
    pickup = nothing & np.isin(t, (KEY, BALL, BOX))
    drop = ~nothing & (t == EMPTY) & ~present
    toggle = (t == BOX) | (door & ((st != LOCKED) | ((ctype == KEY) & (ccol == col)))) | stale | hit
    front = live & inside
    return (3 * live + front * (4 * forward + 8 * pickup + 16 * drop + 32 * toggle)).astype(np.uint8)


def expanded(mask):
    """u8[..., 7] of 0 / 1: byte k = bit k"""
    return ((np.asarray(mask)[..., None] >> np.arange(7)) & 1).astype(np.uint8)


def test_the_model_on_a_worked_example():
    spec = EnvSpec(5, 5, 4, 3, allow_agent_overlap=False)
    g, _ = layouts.empty_layout(5, 1)
    g[1, 2] = (KEY, 1, 0)
    g[2, 1] = (DOOR, 1, LOCKED)
    ag = np.zeros((4, 8), np.uint8)
    ag[:, 5] = EMPTY
    ag[0, 1:4] = (0, 1, 1)                                                   # faces the key: pickup
    ag[1, 1:4] = (2, 2, 2)                                                   # faces the locked door with its key: toggle
    ag[1, 5:7] = (KEY, 1)
    ag[2, 1:4] = (3, 3, 2)                                                   # faces an empty cell, carrying a ball: forward, drop
    ag[2, 5:7] = (BALL, 0)
    ag[3, 1:4] = (1, 3, 0)                                                   # stands ON the border facing in: agent 2 ... is not there
    ag[3, 4] = 1                                                             # ... and it is terminated
    got = model_action_mask(3, g[None], ag[None], None, spec)[0].tolist()
    assert got == [3 | 8, 3 | 32, 3 | 4 | 16, 0]
    ag[3, 1:4] = (1, 3, 1)                                                   # the terminated agent in front of agent 2: it counts
    assert model_action_mask(3, g[None], ag[None], None, spec)[0].tolist() == [3 | 8, 3 | 32, 3, 0]
    ag[0, 1:4] = (2, 0, 1)                                                   # on the border, facing out: the turns alone
    assert model_action_mask(3, g[None], ag[None], None, spec)[0, 0] == 3
    assert expanded(np.uint8(3 | 32)).tolist() == [1, 1, 0, 0, 0, 1, 0]


# ---- random states -----------------------------------------------------------------------------------------------------------------

def random_rows(r, n, W, H, A, cb, kind="empty"):
    """n random states as the model, the host program and the kernel take them: valid cells in the format cb; agents anywhere -- on
    the border facing out too --, a part of them terminated, carrying or standing in front of one another; aux made for the kind"""
    tri = valid_triples(contents=cb != 1)
    g = tri[r.integers(0, len(tri), size=(n, H, W))]
    cells = g if cb == 3 else (layouts.pack_cells8(g) if cb == 1 else layouts.pack_cells(g))
    ag = np.zeros((n, A, 8), np.uint8)
    ag[..., 0] = r.integers(0, 6, size=(n, A))
    ag[..., 1] = r.integers(0, 4, size=(n, A))
    ag[..., 2] = r.integers(0, W, size=(n, A))
    ag[..., 3] = r.integers(0, H, size=(n, A))
    edge = r.random((n, A)) < 0.3                                            # on a border, and mostly facing out
    side = r.integers(0, 4, size=(n, A))
    ag[..., 2] = np.where(edge & (side == 0), W - 1, np.where(edge & (side == 2), 0, ag[..., 2]))
    ag[..., 3] = np.where(edge & (side == 1), H - 1, np.where(edge & (side == 3), 0, ag[..., 3]))
    ag[..., 1] = np.where(edge & (r.random((n, A)) < 0.8), side, ag[..., 1])
    ag[..., 4] = r.random((n, A)) < 0.15
    carried = np.array([(EMPTY, 0, 0)] * 6 + [(t, c, 0) for t in (KEY, BALL, BOX) for c in range(6)] + [(KEY, c, 0) for c in range(6)], np.uint8)
    ag[..., 5:8] = carried[r.integers(0, len(carried), size=(n, A))]
    d = ag[..., 1].astype(np.int64)
    fx = ag[..., 2] + (d == 0).astype(np.int64) - (d == 2).astype(np.int64)
    fy = ag[..., 3] + (d == 1).astype(np.int64) - (d == 3).astype(np.int64)
    ok = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    for a in range(1, A):                                                    # agent a in front of agent a - 1, in a third of the rows
        move = ok[:, a - 1] & (r.random(n) < 0.33)
        ag[move, a, 2], ag[move, a, 3] = fx[move, a - 1], fy[move, a - 1]
    aux = r.integers(0, 256, size=(n, 16), dtype=np.uint8)
    some = np.arange(n), r.integers(0, A, size=n)
    if kind == "redbluedoors":
        aux[:, 0], aux[:, 1] = np.clip(fx[some], 0, 255), np.clip(fy[some], 0, 255)
        aux[:, 4] = r.integers(0, 2, size=n) * r.integers(1, 256, size=n)
    elif kind == "rules":
        aux[:, 0] = r.integers(0, 5, size=n)                                 # (more than MGX_MAX_RULES: as 3)
        for k in range(3):
            aux[:, 1 + 5 * k] = r.integers(1, 3, size=n)
            who = np.arange(n), r.integers(0, A, size=n)
            aux[:, 2 + 5 * k], aux[:, 3 + 5 * k] = np.clip(fx[who], 0, 255), np.clip(fy[who], 0, 255)
    return {"cells": np.ascontiguousarray(cells), "agents": ag, "aux": aux}


def spec_for(W, H, A, cb=2, kind="empty", overlap=True):
    return EnvSpec(W, H, A, 3, allow_agent_overlap=overlap, env_kind=kind, cell_bytes=cb)


# ---- csrc/mgx_action_mask.h, built by g++ into a program of its own ----------------------------------------------------------------

HOST_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mgx_action_mask.h"
#include "mgx_aux_geom.h"
using namespace mgx;
static long long rd(FILE *f) { long long v = 0; if (fread(&v, 8, 1, f) != 1) return -1; return v; }
static std::vector<uint8_t> bytes(FILE *f, size_t n) {
    std::vector<uint8_t> b(n);
    if (n && fread(b.data(), 1, n, f) != n) { printf("short input\n"); exit(2); }
    return b;
}
static uint64_t make_row(int color, int dir, int x, int y, int term, uint32_t carry) {
    return (uint64_t)color | (uint64_t)dir << 8 | (uint64_t)x << 16 | (uint64_t)y << 24 | (uint64_t)term << 32 | (uint64_t)carry << 40;
}
// Every front cell x carry x presence x overlap setting x stale flag x direction, in both packed formats: the mask of
// action_mask_host against eval_agent's `go && (nrow != row || writes)` for the actions 0..5 (and `done`, which does nothing).
static long long exhaustive() {
    long long checked = 0;
    std::vector<uint32_t> carries;
    for (uint32_t t = 0; t <= 10; ++t)
        for (uint32_t c = 0; c < 6; ++c) carries.push_back(t | c << 8);
    carries.push_back((uint32_t)T_BOX | 2u << 8 | (1u | 3u << 3) << 18);         // a carried box that holds something
    for (int cb = 1; cb <= 2; ++cb) {
        std::vector<uint32_t> cells;                                             // raw cells of the format
        if (cb == 2) {
            for (uint32_t t = 0; t <= 10; ++t)
                for (uint32_t c = 0; c < 6; ++c)
                    for (uint32_t s = 0; s < 4; ++s) {
                        cells.push_back(cell_pack(t | c << 8 | s << 16));
                        if (t == (uint32_t)T_BOX)
                            for (uint32_t kind = 1; kind < 8; ++kind) cells.push_back(cell_pack(t | c << 8 | s << 16 | (kind | (c ^ 1u) << 3) << 18));
                    }
        } else {
            for (uint32_t tc = 0; tc < 16; ++tc)
                for (uint32_t c = 0; c < 6; ++c) cells.push_back(cell8_pack(cell8_unpack(tc | c << 4)));
        }
        for (int d = 0; d < 4; ++d) {
            const int fx = 1 + dir_dx(d), fy = 1 + dir_dy(d);
            for (uint32_t raw : cells)
                for (uint32_t carry : carries)
                    for (int present = 0; present < 3; ++present)               // nobody there; a live agent; a terminated one
                        for (int overlap = 0; overlap < 2; ++overlap)
                            for (int stale = 0; stale < 2; ++stale)
                                for (int term = 0; term < 2; ++term) {
                                    MgxSpec sp;
                                    memset(&sp, 0, sizeof sp);
                                    sp.width = 3; sp.height = 3; sp.num_agents = 2; sp.view_size = 3; sp.max_steps = 10;
                                    sp.allow_agent_overlap = overlap; sp.env_kind = MGX_KIND_REDBLUEDOORS; sp.cell_bytes = cb;
                                    const StepCfg cf = make_cfg(sp);
                                    std::vector<uint16_t> store(9, 0);           // (2-byte aligned for the 16-bit cells)
                                    uint8_t *tile = reinterpret_cast<uint8_t *>(store.data());
                                    for (int p = 0; p < 9; ++p) store_cell_raw(cb, tile + p * cb, cb == 1 ? CELL8_WALL : CELL16_WALL);
                                    store_cell_raw(cb, tile + 4 * cb, cb == 1 ? cell8_pack(CELL_EMPTY) : cell_pack(CELL_EMPTY));
                                    const int off = (fy * 3 + fx) * cb;
                                    store_cell_raw(cb, tile + off, raw);
                                    uint64_t rows[2] = {make_row(1, d, 1, 1, term, carry),
                                                        present ? make_row(2, 0, fx, fy, present == 2, CELL_EMPTY) : make_row(2, 0, 1, 1, 0, CELL_EMPTY)};
                                    uint8_t aux[16] = {(uint8_t)fx, (uint8_t)fy, 0, 0, (uint8_t)stale};
                                    uint8_t mask[2];
                                    action_mask_host(sp, cb, tile, reinterpret_cast<const uint8_t *>(rows), aux, mask);
                                    if (mask[0] & 0xC0) { printf("FAILED high bits\n"); return -1; }
                                    for (int act = 0; act <= ACT_DONE; ++act) {
                                        const AgentEval ev = eval_agent(cf, tile, rows, act, rows[0], true, stale_offset(cf, aux, sp.env_kind));
                                        const bool want = ev.go && (ev.nrow != rows[0] || ev.writes);
                                        if (want != (bool)((mask[0] >> act) & 1)) {
                                            printf("FAILED cb %d dir %d cell %x carry %x present %d overlap %d stale %d term %d action %d: eval_agent %d\n",
                                                   cb, d, raw, carry, present, overlap, stale, term, act, (int)want);
                                            return -1;
                                        }
                                        ++checked;
                                    }
                                }
        }
    }
    return checked;
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    for (long long kind; (kind = rd(f)) >= 0;) {
        if (kind == 0) {                                   // states: W H A cb n has_aux env_kind overlap, then cells, agents, aux
            MgxSpec sp;
            memset(&sp, 0, sizeof sp);
            sp.width = (int)rd(f); sp.height = (int)rd(f); sp.num_agents = (int)rd(f);
            const int cb = (int)rd(f), n = (int)rd(f), has_aux = (int)rd(f);
            sp.env_kind = (int)rd(f); sp.allow_agent_overlap = (int)rd(f); sp.cell_bytes = cb; sp.view_size = 3;
            const int A = sp.num_agents;
            const size_t tile = (size_t)sp.width * sp.height * cb;
            const auto cells = bytes(f, tile * n), agents = bytes(f, (size_t)n * A * 8), aux = bytes(f, has_aux ? (size_t)n * 16 : 0);
            for (int i = 0; i < n; ++i) {
                std::vector<uint8_t> tile_i(cells.begin() + i * tile, cells.begin() + (i + 1) * tile);   // (their own allocations:
                std::vector<uint8_t> ag(agents.begin() + (size_t)i * A * 8, agents.begin() + (size_t)(i + 1) * A * 8);   //  an over-read shows)
                std::vector<uint8_t> ax, mask(A, 0xEE);
                if (has_aux) ax.assign(aux.begin() + i * 16, aux.begin() + (i + 1) * 16);
                action_mask_host(sp, cb, tile_i.data(), ag.data(), has_aux ? ax.data() : nullptr, mask.data());
                for (int a = 0; a < A; ++a) printf("%02x", mask[a]);
                printf(" ");
                for (int t = 0; t < kMaskActions * A; ++t) printf("%d", (int)mask_expand_byte(mask[mask_expand_agent(t)], t));
                printf("\n");
            }
        } else if (kind == 1) {                            // the exhaustive table
            const long long c = exhaustive();
            if (c < 0) return 1;
            printf("exhaustive %lld\n", c);
        } else {                                           // geometry: A n
            const int A = (int)rd(f);
            const long long n = rd(f);
            const ActionMaskGeom g = action_mask_geom(A, n);
            if (g.group < A || (g.group & (g.group - 1)) || (g.group > 1 && g.group / 2 >= A) || g.per * g.group != 64
                || g.nwaves * g.per < n || (g.nwaves - 1) * g.per >= n || g.blocks * kMaskWpb < g.nwaves
                || (g.blocks - 1) * kMaskWpb >= g.nwaves) { printf("FAILED geometry\n"); return 1; }
            printf("%d %d %lld %lld\n", g.group, g.per, (long long)g.nwaves, (long long)g.blocks);
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
    d = tmp_path_factory.mktemp("action_mask_host")
    src = d / "action_mask_host.cpp"
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


def states_payload(spec, cb, rows, aux=True):
    n = rows["agents"].shape[0]
    head = _i64(0, spec.width, spec.height, spec.num_agents, cb, n, int(aux), KINDS[spec.env_kind], int(spec.allow_agent_overlap))
    return head + rows["cells"].tobytes() + rows["agents"].tobytes() + (rows["aux"].tobytes() if aux else b"")


def mask_lines(mask):
    """what the host program prints for masks u8[n,A]: the bytes in hex, then the expanded form"""
    return ["".join(f"{int(m):02x}" for m in row) + " " + "".join(str(int(b)) for b in expanded(row).reshape(-1)) for row in mask]


HOST_SHAPES = ((3, 3), (5, 5), (7, 6), (16, 16))


@pytest.fixture(scope="module")
def host_cases():
    """(payload, expected lines, the masks) over shapes, agent counts, formats, env kinds and the overlap setting"""
    r = np.random.default_rng(21)
    payload, want, masks = [], [], []
    for W, H in HOST_SHAPES:
        for A in (1, 3, 4, 32):
            for cb in (2, 1, 3):
                for j, kind in enumerate(("empty", "redbluedoors", "rules")):
                    spec = spec_for(W, H, A, cb, kind, overlap=bool((A + cb + j) % 2))
                    has_aux = kind != "empty" or bool(cb % 2)                 # (a set without aux: where no hook reads it)
                    rows = random_rows(r, 12, W, H, A, cb, kind)
                    m = model_action_mask(cb, rows["cells"], rows["agents"], rows["aux"] if has_aux else None, spec)
                    payload.append(states_payload(spec, cb, rows, has_aux))
                    want += mask_lines(m)
                    masks.append(m.reshape(-1))
    return b"".join(payload), want, np.concatenate(masks)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_header_gives_the_models_masks(host_programs, host_cases, which):
    payload, want, masks = host_cases
    got = host_programs(which, payload)
    assert len(got) == len(want) == 4 * 4 * 3 * 3 * 12
    assert got == want
    # the random states are not hollow: every bit both ways, terminated agents, and nothing above bit 5
    assert (masks & 0xC0 == 0).all() and (masks == 0).sum() > 100
    for bit in range(6):
        on = ((masks >> bit) & 1).astype(bool)
        off = int((~on & (masks != 0)).sum())                               # (clear on a live agent: never for the turns)
        assert on.sum() > 100 and (off == 0 if bit < 2 else off > 100), bit


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_header_agrees_with_eval_agent_on_every_front_cell(host_programs, which):
    """the table runs inside the program (HOST_MAIN: exhaustive): 16-bit cells 11 types x 6 colours x 4 states + the boxes' contents,
    compact cells 16 codes x 6 colours; 67 carries; 3 presences; 2 overlap settings; stale or not; terminated or not; 4 directions;
    7 actions"""
    got = host_programs(which, _i64(1))
    cells = (11 * 6 * 4 + 6 * 4 * 7) + 16 * 6
    assert got == [f"exhaustive {cells * 4 * 67 * 3 * 2 * 2 * 2 * 7}"]


def hook_examples():
    """the two hook clauses, by hand: [(spec, rows of ONE env in byte triples -- aux may be None --, its masks)], the same state with
    and without the stale flag / the rule / any aux at all.  Agent 0 faces the blue door (open in the grid), agent 1 an empty cell."""
    g, _ = layouts.empty_layout(5, 1)
    g[2, 3] = (DOOR, 2, OPEN)
    ag = np.zeros((1, 2, 8), np.uint8)
    ag[..., 5] = EMPTY
    ag[0, 0, 1:4] = (0, 2, 2)
    ag[0, 1, 1:4] = (1, 1, 1)
    plain = [3 | 4 | 32, 3 | 4]
    out = []
    for kind, aux_on, with_hook in (
            ("redbluedoors", [3, 2, 0, 0, 1], [3 | 32, 3 | 4]),              # the object is closed: no forward; toggle either way
            ("rules", list(layouts.rules_aux([("toggles_at", 1, 2, "failure")])), [3 | 4 | 32, 3 | 4 | 32])):   # agent 1's empty front cell
        spec = spec_for(5, 5, 2, 3, kind)
        aux_off = aux_on[:4] if kind == "redbluedoors" else [0] + aux_on[1:]     # the flag down; the table declared empty
        for aux, want in ((aux_on, with_hook), (aux_off, plain), (None, plain)):
            a = None
            if aux is not None:
                a = np.zeros((1, 16), np.uint8)
                a[0, :len(aux)] = aux
            out.append((spec, {"cells": g[None].copy(), "agents": ag.copy(), "aux": a}, [want]))
    return out


def test_a_stale_door_and_a_rule_change_the_mask(host_programs):
    for spec, rows, want in hook_examples():
        m = model_action_mask(3, rows["cells"], rows["agents"], rows["aux"], spec)
        assert m.tolist() == want, (spec.env_kind, rows["aux"])
        assert host_programs("sanitized", states_payload(spec, 3, rows, aux=rows["aux"] is not None)) == mask_lines(m)


def geometry(A, n):
    """(group, per, wavefronts, workgroups) of a mgx_action_mask launch: csrc/mgx_aux_geom.h restated (held to it below)"""
    group = 1
    while group < A:
        group *= 2
    per = 64 // group
    nwaves = (n + per - 1) // per
    return group, per, nwaves, (nwaves + 3) // 4


def test_the_launch_geometry_is_what_the_gpu_tests_name(host_programs):
    cases = [(A, n) for A in range(1, 33) for n in (1, 2, 63, 64, 65, 255, 257, 65536, (1 << 31) + 1)]
    got = host_programs("sanitized", b"".join(_i64(2, *c) for c in cases))
    assert [tuple(int(v) for v in ln.split()) for ln in got] == [geometry(*c) for c in cases]
    assert [geometry(A, 70)[0] for A in (1, 2, 3, 5, 32)] == [1, 2, 4, 8, 32]


# ---- sound and tight, against the oracle on reachable states -----------------------------------------------------------------------

WALK_ENVS, WALK_MAX = 40, 40
WALK_WEIGHTS = [LEFT, RIGHT, FORWARD, FORWARD, FORWARD, PICKUP, PICKUP, DROP, TOGGLE, TOGGLE, DONE]


def _walk_class(ci):
    """(spec, start state) of env class ci: WALK_ENVS generator resets (layouts.*_layout: the reference's _gen_grid restated), or the
    hook-dense RULES states of tests/hook_states.py (a toggles_at rule)"""
    grids, agents, auxs = [], [], []
    if ci == 5:
        c = hook_states.case("rules_fetchtrap_a2_v7")
        st = {k: v[:WALK_ENVS].copy() for k, v in c.state.items()}
        st["step_count"][:] = 0
        return c.spec, st
    for s in range(WALK_ENVS):
        lr, nr = np.random.default_rng(1000 * ci + s), np.random.default_rng(5000 * ci + s)
        if ci == 0:
            spec = EnvSpec(6, 6, 3, 3, max_steps=200, allow_agent_overlap=False, success_termination_mode="all")
            g, a = layouts.empty_layout(6, 3, None, None, lr)
            aux = np.zeros(16, np.uint8)
        elif ci == 1:
            spec = EnvSpec(11, 6, 2, 3, max_steps=200, env_kind="blockedunlockpickup")
            g, a, tgt = layouts.blockedunlockpickup_layout(6, 2, lr, nr)
            aux = layouts.make_aux("blockedunlockpickup", g, tgt)
        elif ci == 2:
            spec = EnvSpec(12, 6, 2, 3, max_steps=200, env_kind="redbluedoors", failure_termination_mode="all")
            g, a = layouts.redbluedoors_layout(6, 2, lr)
            aux = layouts.make_aux("redbluedoors", g)
        elif ci == 3:
            spec = EnvSpec(13, 5, 3, 3, max_steps=200, allow_agent_overlap=False, env_kind="lockedhallway")
            g, a = layouts.lockedhallway_layout(2, 5, 1, 2, 3, lr, nr)
            aux = layouts.make_aux("lockedhallway", g)
        else:
            spec = EnvSpec(13, 13, 3, 3, max_steps=200, allow_agent_overlap=False)
            g, a = layouts.playground_layout(5, 3, 3, 3, lr, nr)
            aux = np.zeros(16, np.uint8)
        grids.append(g); agents.append(a); auxs.append(aux)
    B = WALK_ENVS
    rng = np.random.default_rng(31 + ci).integers(0, 2 ** 63, size=(B, 4), dtype=np.int64).astype(np.uint64)
    rng[:, 2] |= np.uint64(1)
    return spec, dict(grid=np.ascontiguousarray(np.stack(grids)), agents=np.ascontiguousarray(np.stack(agents)), rng=rng,
                      step_count=np.zeros(B, np.int32), aux=np.ascontiguousarray(np.stack(auxs)))


STATE = ("grid", "agents", "rng", "step_count", "aux")


def _oracle_step(spec, st, acts):
    """(outputs, post-state) of one oracle step of a copy of `st`"""
    from oracle import binding as ob
    s = {k: v.copy() for k, v in st.items()}
    out = ob.step_batch(spec.as_dict(), s["grid"], s["agents"], s["rng"], s["step_count"], np.ascontiguousarray(acts), s["aux"])
    return [o.copy() for o in out], s


@pytest.fixture(scope="module")
def walked():
    """per env class: (spec, the states after random walks of 0..WALK_MAX steps -- env b of the batch is kept as it is after
    lengths[b] steps)"""
    from oracle import binding as ob
    out = []
    for ci in range(6):
        spec, st = _walk_class(ci)
        r = np.random.default_rng(77 + ci)
        B, A = st["agents"].shape[:2]
        lengths = r.integers(0, WALK_MAX + 1, size=B)
        lengths[:2] = (0, WALK_MAX)
        kept = {k: v.copy() for k, v in st.items()}
        for t in range(1, WALK_MAX + 1):
            acts = r.choice(np.array(WALK_WEIGHTS, np.int8), size=(B, A)).astype(np.int8)
            ob.step_batch(spec.as_dict(), st["grid"], st["agents"], st["rng"], st["step_count"], acts, st["aux"])
            for k in STATE:
                kept[k][lengths == t] = st[k][lengths == t]
        assert (kept["step_count"] == lengths).all()
        out.append((spec, kept))
    return out


def test_the_mask_is_sound_and_tight_against_the_oracle(walked, host_programs):
    census = {"set": np.zeros(6, np.int64), "clear": np.zeros(6, np.int64), "terminated": 0, "blocked": 0}
    for spec, st in walked:
        B, A = st["agents"].shape[:2]
        mask = model_action_mask(3, st["grid"], st["agents"], st["aux"], spec)
        rows = {"cells": st["grid"], "agents": st["agents"], "aux": st["aux"]}
        assert host_programs("plain", states_payload(spec, 3, rows)) == mask_lines(mask)      # the header's masks are these masks
        live = st["agents"][..., 4] == 0
        census["terminated"] += int((~live).sum())
        assert (mask[~live] == 0).all()
        with_overlap = model_action_mask(3, st["grid"], st["agents"], st["aux"], EnvSpec.from_dict(dict(spec.as_dict(), allow_agent_overlap=True)))
        census["blocked"] += int((live & (mask & 4 == 0) & (with_overlap & 4 != 0)).sum())
        done = np.full((B, A), DONE, np.int8)
        base_out, base_post = _oracle_step(spec, st, done)
        for a in range(A):
            for act in range(6):
                acts = done.copy()
                acts[:, a] = act
                out, post = _oracle_step(spec, st, acts)
                same_out = np.array([all(o[b].tobytes() == p[b].tobytes() for o, p in zip(out, base_out)) for b in range(B)])
                same = {k: np.array([post[k][b].tobytes() == base_post[k][b].tobytes() for b in range(B)]) for k in STATE}
                bit = ((mask[:, a] >> act) & 1).astype(bool)
                on, off = live[:, a] & bit, live[:, a] & ~bit
                census["set"][act] += int(on.sum())
                census["clear"][act] += int(off.sum())
                everything = same_out & np.logical_and.reduce([same[k] for k in STATE])
                assert everything[off].all(), (spec.env_kind, a, act, np.flatnonzero(off & ~everything)[:5])           # sound
                if spec.env_kind != "rules":
                    moved = ~(same["grid"] & same["agents"])
                    assert moved[on].all(), (spec.env_kind, a, act, np.flatnonzero(on & ~moved)[:5])                  # tight
    print("census", {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in census.items()})
    assert (census["set"][2:] > 0).all() and (census["clear"][2:] > 0).all(), census
    assert (census["set"][:2] > 0).all() and census["terminated"] > 0 and census["blocked"] > 0, census


# ---- the Python layer over the model -----------------------------------------------------------------------------------------------

class MaskOracle(CopyOracle):
    """the oracle launcher + env_copy (the model of tests/test_env_snapshot.py) + action_mask, which is the model above;
    `mask_calls` records (n, members, flags)."""

    def __init__(self, spec):
        super().__init__(spec)
        self.mask_calls = []

    def action_mask(self, n, rows, n_rows, idx, flags, mask, bad):
        self.mask_calls.append((n, sorted(k for k, v in rows.items() if v is not None), flags))
        r = self._np(rows)
        assert tuple(mask.shape) == ((n, self.spec.num_agents, 7) if flags & EXPAND else (n, self.spec.num_agents))
        assert mask.dtype is (torch.bool if flags & EXPAND else torch.uint8)
        for i in range(n):
            s = i if idx is None else int(idx[i])
            if not 0 <= s < n_rows:
                if bad is not None:
                    bad[0] += 1
                    bad[1] = min(int(bad[1]), min(i, INT32_MAX))
                continue
            m = model_action_mask(cell_bytes_of(self.spec), r["cells"][s:s + 1], r["agents"][s:s + 1],
                                  r["aux"][s:s + 1] if "aux" in r else None, self.spec)[0]
            mask[i] = torch.from_numpy(expanded(m).astype(bool) if flags & EXPAND else m)


SPEC = EnvSpec(5, 5, 2, 3, max_steps=6, allow_agent_overlap=False)


def env_masks(env):
    """the model on what the env shows: .grid (byte triples), agents, aux"""
    return model_action_mask(3, env.grid.cpu().numpy(), env.agents.cpu().numpy(), env.aux.cpu().numpy(), env.spec)


def test_action_mask_of_a_batch_and_its_arguments():
    B, A = 7, 2
    be = MaskOracle(SPEC)
    env = make_env("pool", B=B, spec=SPEC, backend=be)
    for a in actions_for(B, A, 3, 4):
        env.step(a, auto_reset=True)
    mask = env.action_mask()
    assert mask.dtype is torch.uint8 and tuple(mask.shape) == (B, A) and mask.device == env.device
    assert mask.numpy().tolist() == env_masks(env).tolist()
    assert len(np.unique(mask.numpy())) > 1
    assert be.mask_calls[-1] == (B, ["agents", "aux", "cells"], 0)
    wide = env.action_mask(expand=True)
    assert wide.dtype is torch.bool and tuple(wide.shape) == (B, A, 7) and be.mask_calls[-1][2] == EXPAND
    assert wide.numpy().tolist() == expanded(mask.numpy()).astype(bool).tolist() and not wide[..., 6].any()
    # chosen envs, repeats allowed; out= is written and handed back
    ids = torch.tensor([6, 0, 0, 3])
    out = torch.full((4, A), 0xAA, dtype=torch.uint8)
    assert env.action_mask(ids, out=out) is out and out.tolist() == mask[ids].tolist()
    out = torch.zeros((4, A, 7), dtype=torch.bool)
    assert env.action_mask(ids, expand=True, out=out) is out and out.tolist() == wide[ids].tolist()
    assert env.action_mask(torch.zeros(0, dtype=torch.int64)).shape == (0, A)
    # refusals
    for t in (torch.arange(4, dtype=torch.int32), torch.arange(4).reshape(2, 2), torch.arange(8)[::2], [0, 1]):
        with pytest.raises(ValueError, match="env_ids must be a contiguous int64 tensor"):
            env.action_mask(t)
    for bad_out in (torch.zeros((B, A), dtype=torch.int8), torch.zeros((B, A), dtype=torch.bool), torch.zeros((B + 1, A), dtype=torch.uint8),
                    torch.zeros((B, A, 7), dtype=torch.uint8), torch.zeros((B, 2 * A), dtype=torch.uint8)[:, ::2], np.zeros((B, A), np.uint8)):
        with pytest.raises(ValueError, match="out= must be a contiguous uint8 tensor of shape"):
            env.action_mask(out=bad_out)
    for bad_out in (torch.zeros((B, A, 7), dtype=torch.uint8), torch.zeros((B, A), dtype=torch.bool), torch.zeros((B, A, 8), dtype=torch.bool)):
        with pytest.raises(ValueError, match="out= must be a contiguous bool tensor of shape"):
            env.action_mask(expand=True, out=bad_out)
    with pytest.raises(ValueError, match="out= must be a contiguous uint8 tensor of shape"):
        env.action_mask(ids, out=torch.zeros((B, A), dtype=torch.uint8))
    env._session = object()
    with pytest.raises(RuntimeError, match="persistent session"):
        env.action_mask()
    env._session = None
    with pytest.raises(RuntimeError, match="no state loaded"):
        BatchedMultiGridEnv(SPEC, B, "cpu", backend=MaskOracle(SPEC)).action_mask()
    with pytest.raises(RuntimeError, match="sub-shard of split"):
        env.split(2)[0].action_mask()
    # ids out of range: their masks are left alone, and check_errors() tells -- in the words it has for snapshots
    out = torch.full((4, A), 0xAA, dtype=torch.uint8)
    env.action_mask(torch.tensor([1, B, -1, 2]), out=out)
    assert out.tolist() == [mask[1].tolist(), [0xAA] * A, [0xAA] * A, mask[2].tolist()]
    with pytest.raises(ValueError, match=r"2 pair\(s\) named an env id or a snapshot row out of range.*first at pair 1"):
        env.check_errors()
    env.check_errors()


def test_a_snapshots_rows_have_the_masks_of_their_moment():
    B, A = 40, 2
    env = make_env("pool", B=B, spec=SPEC, backend=MaskOracle(SPEC))
    for a in actions_for(B, A, 3, 4):
        env.step(a, auto_reset=True)
    snap = env.snapshot()
    at_snap = env.action_mask()
    for a in actions_for(B, A, 2, 9):
        env.step(a, auto_reset=True)
    assert (env.action_mask() != at_snap).any()
    assert snap.action_mask().tolist() == at_snap.tolist()
    assert env.backend.mask_calls[-1] == (B, ["agents", "aux", "cells"], 0)
    rows = torch.tensor([3, 3, 39])
    out = torch.zeros((3, A, 7), dtype=torch.bool)
    assert snap.action_mask(rows, expand=True, out=out) is out
    assert out.numpy().tolist() == expanded(at_snap[rows].numpy()).astype(bool).tolist()
    env.restore(snap)
    assert env.action_mask().tolist() == at_snap.tolist()
    # a snapshot row out of range is reported by the env that took the snapshot
    snap.action_mask(torch.tensor([0, B]))
    with pytest.raises(ValueError, match=r"1 pair\(s\) named an env id or a snapshot row out of range.*first at pair 1"):
        env.check_errors()
    with pytest.raises(ValueError, match="rows must be a contiguous int64 tensor"):
        snap.action_mask(torch.arange(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="out= must be a contiguous uint8 tensor of shape"):
        snap.action_mask(rows, out=torch.zeros((B, A), dtype=torch.uint8))
    del env
    gc.collect()
    with pytest.raises(RuntimeError, match="the env this snapshot was taken from is gone"):
        snap.action_mask()


def test_the_layout_marker_stays_armed_across_a_mask():
    B = 7
    env = make_env("pool", B=B, spec=SPEC, backend=MaskOracle(SPEC), pool_size=1)
    assert env._tracks() and env._mark["armed"] and env._marker.tolist() == [0] * B
    before = {k: getattr(env, k).clone() for k in ("_marker", "rng", "step_count", "episode")}
    env.action_mask()
    env.action_mask(torch.tensor([1, 2]), expand=True)
    assert env._mark["armed"] and all((getattr(env, k) == v).all() for k, v in before.items())


def test_sixteen_bit_and_compact_envs_in_step_have_equal_masks():
    B, T = 7, 8
    envs = []
    for cb in (2, 1):
        spec = EnvSpec(5, 5, 2, 3, max_steps=6, cell_bytes=cb, allow_agent_overlap=False)
        env = BatchedMultiGridEnv(spec, B, "cpu", backend=MaskOracle(spec))
        pg, pa = empty_pool(spec)
        env.load_state(pg[0], pa[0])
        env.seed(3)
        envs.append(env)
    assert envs[0]._cells.dtype is torch.int16 and envs[1]._cells.dtype is torch.uint8
    seen = set()
    for a in actions_for(B, 2, T, 2):
        masks = [env.action_mask() for env in envs]
        assert masks[0].tolist() == masks[1].tolist() == env_masks(envs[0]).tolist()
        seen |= set(masks[0].reshape(-1).tolist())
        for env in envs:
            env.step(a)
    assert {3, 3 | 4} <= seen                                                # (an Empty grid: `forward` blocked, and not)


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------------

def test_c_abi_argument_validation():
    """what mgx_action_mask checks of its own; the checks of every row query: tests/test_row_query_abi.py"""
    from tests.test_row_query_abi import INV, UNS, P as p, full, ref
    L = _lib.lib()
    sc = EnvSpec(5, 5, 2, 3, max_steps=4).to_c()

    def M(sc_, n, src, idx=p, flags=1, mask=p + 1, bad=p):
        return L.mgx_action_mask(ref(sc_), n, ref(src), idx, flags, mask, bad, None)
    a = full()
    for flags in (2, 3, 8, 0x80000000):
        assert M(sc, 4, a, flags=flags) == INV and M(sc, 0, a, flags=flags) == INV
    assert M(sc, 4, a, mask=None) == INV
    big = EnvSpec(5, 5, 2, 3).to_c()
    big.width, big.height = 1024, 129
    assert M(big, 4, a) == UNS


def test_the_export_is_the_headers_declaration():
    from tests.test_capi import declared_functions
    names = declared_functions()
    assert "mgx_action_mask" in names and "mgx_action_mask" in _lib.EXPORTS and getattr(_lib.lib(), "mgx_action_mask") is not None
    assert set(names) == set(_lib.EXPORTS) and _lib.lib().mgx_abi_version() == _lib.ABI_VERSION == 11
    assert _lib.MASK_EXPAND == EXPAND
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "ACTION MASKS" in hdr and "MGX_MASK_EXPAND = 1" in hdr
    from multigrid_amd import build
    assert os.path.join(build.CSRC, "mgx_action_mask.h") in build.DEPS and any(u[0] == "mgx_action_mask" for u in build.UNITS)
