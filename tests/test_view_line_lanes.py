"""CPU check of the line map of the one-step kernels' P2 / P4 (mgx_fused.h gather_lines; mgx_rules.h "line map"): eight lanes per
view slot, lane (slot, j) owns view row j.  A g++ build of mgx_rules.h -- the device instructions restated for the host -- compares
the line map with the cell map it replaces, piece by piece:

  * the tile address of every cell: line_base + line_cell_offset against clamped_offset (v_pk_max_i16 / v_pk_min_i16 /
    v_dot2_i32_i16 restated), with the view record exactly as P1d writes it, for V in {3, 5, 7}, every agent position of an 8x8,
    an 11x6 and a 16x16 grid including the positions on and outside the border, all four directions, row pitch W and W - 1;
  * the see-behind bytes folded per line (line_opaque_byte), read back as one word and flooded (vis_mask_lines), against vis_mask
    on the cell map's word k = j*V + i, bit for bit, on random opacity patterns and with the own cell patched either way;
  * mask + unpack of a line (line_stage_cell) against the staged dword of the cell map's P4 (bytes 0-2), both halves of a pair.

Every case is checked.  The GPU parity tests (test_view_line_lanes_gpu.py and the existing ones) run the kernels themselves."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdint>
#include <initializer_list>
#include "multigrid_amd/csrc/mgx_rules.h"
using namespace mgx;

static uint64_t rs = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 16); }

struct Rec { int origin; uint32_t steps, lo, hi; };           // mgx_fused.h ViewRec

// the offsets of a line's V cells, as gather_lines / line_reads compute them
template <int V, int I>
static void line_offsets(const Rec &r, int base, int (&off)[V]) {
    if constexpr (I < V) {
        off[I] = line_cell_offset<I - V / 2>(base, clamp_hi16(r.lo), clamp_hi16(r.hi), clamp_hi16(r.steps));
        line_offsets<V, I + 1>(r, base, off);
    }
}

static long n_addr = 0, n_vis = 0, n_stage = 0;

template <int V>
static int addresses(int W, int H, int pitch) {
    constexpr int kWall = 1 << 20;                                  // the wavefront's WALL cell (an address outside any tile)
    int bad = 0;
    for (int x = 0; x <= W + 1; ++x)                                // x = W, W + 1 and y = H, H + 1: outside the grid
        for (int y = 0; y <= H + 1; ++y)
            for (int d = 0; d < 4; ++d) {
                const ViewGeom g = view_geom<V>(W, H, x, y, d, kCellBytes, pitch);
                const ViewClamp vc = view_clamp<V>(g, W, H, x, y);
                Rec r;                                              // mgx_fused_body.inc P1d
                r.origin = vc.valid ? 4096 + g.origin : kWall;
                r.steps = vc.valid ? vc.steps : 0u; r.lo = vc.valid ? vc.lo : 0u; r.hi = vc.valid ? vc.hi : 0u;
                const ViewClamp rc{r.steps, r.lo, r.hi, true};
                for (int j = 0; j < kLineLanes; ++j) {              // the idle lanes j >= V gather too: their reads must stay inside
                    int off[V];
                    line_offsets<V, 0>(r, line_base(r.origin, r.steps, r.lo, r.hi, V - 1 - j), off);
                    for (int i = 0; i < V; ++i) {
                        const int fw = j < V ? V - 1 - j : 0;       // (an idle lane's negative distance clamps to the agent's row)
                        const int want = clamped_offset(r.origin, rc, fw, i - V / 2);
                        ++n_addr;
                        if (off[i] != want && bad++ < 4)
                            std::printf("V=%d %dx%d pitch=%d pos=(%d,%d) dir=%d cell (i=%d, j=%d): %d != %d\n", V, W, H, pitch, x, y, d, i, j,
                                        off[i], want);
                    }
                }
            }
    return bad;
}

// one view: V*V packed 16-bit cells in image order [i][j]
template <int V>
static int view(uint32_t opaque_per_mille) {
    constexpr int NP = (V + 1) / 2;
    uint32_t img[V][V];
    for (int i = 0; i < V; ++i)
        for (int j = 0; j < V; ++j) {
            const uint32_t t = rnd() % 11, col = rnd() % 6, st = rnd() % 3, op = rnd() % 1000 < opaque_per_mille;
            img[i][j] = t | (col << 8) | (st << 12) | (op << 15);   // MgxCell: type | color << 8 | state << 12 | opaque << 15
        }
    int bad = 0;
    // P2: the lines' pair registers and see-behind bytes; LDS bytes[slot][8], byte 7 = the idle lane's junk
    uint32_t pr[V][NP];
    uint64_t word = 0;
    for (int j = 0; j < kLineLanes; ++j) {
        uint32_t b = rnd() & 0xffu;
        if (j < V) {
            for (int k = 0; k < NP; ++k) pr[j][k] = img[2 * k][j] | (2 * k + 1 < V ? img[2 * k + 1][j] << 16 : 0u);
            b = line_opaque_byte<V>(pr[j]);
            uint32_t want = 0;
            for (int i = 0; i < V; ++i) want |= (img[i][j] >> 15) << i;
            if (b != want && bad++ < 4) std::printf("V=%d line %d: opaque byte %02x != %02x\n", V, j, b, want);
        }
        word |= (uint64_t)b << (8 * j);
    }
    // the cell map's ballot word: bit k = j*V + i set = the cell can be seen through (v_cmp_lt_i16 -1, cell)
    uint64_t sbc[1] = {0};
    for (int j = 0; j < V; ++j)
        for (int i = 0; i < V; ++i) sbc[0] |= (uint64_t)(((img[i][j] >> 15) & 1u) ^ 1u) << (j * V + i);
    for (int carry = 0; carry < 2; ++carry) {                       // P3: the own cell's bit patched from what the agent carries
        constexpr int kOwn = (V - 1) * V + V / 2;
        uint64_t a[1] = {(sbc[0] & ~(1ull << kOwn)) | ((uint64_t)carry << kOwn)}, visc[1];
        vis_mask<V, 1>(a, visc);
        // the line map's bytes hold the OPAQUE bits: gather_lines stores them, P3 floods ...
        const uint64_t sbl = (~word & ~(1ull << kLineOwnBit<V>)) | ((uint64_t)carry << kLineOwnBit<V>);
        const uint64_t visl = vis_mask_lines<V>(sbl);
        ++n_vis;
        for (int j = 0; j < kLineLanes; ++j)
            for (int i = 0; i < kLineLanes; ++i) {
                const uint32_t got = (uint32_t)(visl >> (8 * j + i)) & 1u;
                const uint32_t want = (i < V && j < V) ? (uint32_t)(visc[0] >> (j * V + i)) & 1u : 0u;
                if (got != want && bad++ < 4) std::printf("V=%d carry=%d: visibility of (i=%d, j=%d): %u != %u\n", V, carry, i, j, got, want);
            }
        // P4: lane (slot, j) masks and unpacks its line; the cell map stages perm(...) of the slot's half, 0 when unseen
        for (int j = 0; j < V; ++j) {
            const uint32_t vb = (uint32_t)(visl >> (8 * j)) & 0xffu;
            for (int i = 0; i < V; ++i) {
                const uint32_t x = pr[j][i >> 1];
                const uint32_t got = line_stage_cell(x & 0x070f070fu, (x >> 12) & 0x00030003u, i, vb);
                const bool seen = (visc[0] >> (j * V + i)) & 1u;
                for (int half = 0; half < 2; ++half) {              // the cell map: this cell in either half of a register of two slots
                    const uint32_t other = rnd() & 0xffffu;
                    const uint32_t y = half ? (other | (img[i][j] << 16)) : (img[i][j] | (other << 16));
                    const uint32_t c = perm_b32((y >> 12) & 0x00030003u, y & 0x070f070fu, obs_stage_sel(half != 0));
                    const uint32_t want = seen ? c : 0u;
                    ++n_stage;
                    if ((got & 0xffffffu) != (want & 0xffffffu) && bad++ < 4)
                        std::printf("V=%d cell (i=%d, j=%d) half=%d: staged %06x != %06x\n", V, i, j, half, got & 0xffffffu, want & 0xffffffu);
                }
                const uint32_t u = cell_unpack(img[i][j]);
                if ((got & 0xffffffu) != (seen ? u : CELL_UNSEEN) && bad++ < 4)
                    std::printf("V=%d cell (i=%d, j=%d): staged %06x is not the observation's %06x\n", V, i, j, got & 0xffffffu, seen ? u : 0u);
            }
        }
    }
    return bad;
}

template <int V>
static int all() {
    int bad = 0;
    const int grids[3][2] = {{8, 8}, {11, 6}, {16, 16}};
    for (auto &g : grids)
        for (int pitch : {0, g[0] - 1}) bad += addresses<V>(g[0], g[1], pitch);
    for (uint32_t dens : {0u, 100u, 300u, 500u, 800u, 1000u})
        for (int n = 0; n < 2000; ++n) bad += view<V>(dens);
    return bad;
}

int main() {
    const int bad = all<3>() + all<5>() + all<7>();
    std::printf("%ld addresses, %ld floods, %ld staged cells, %d failed\n", n_addr, n_vis, n_stage, bad);
    return bad != 0;
}
"""


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    d = tmp_path_factory.mktemp("view_line_lanes")
    src, exe = d / "line_lanes.cpp", d / "line_lanes"
    src.write_text(SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", f"-I{ROOT}", "-o", str(exe), str(src)])
    return str(exe)


def test_line_map_equals_cell_map(binary):
    p = subprocess.run([binary], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    assert " 0 failed" in p.stdout
    # (nothing sampled away: 3 view sizes x 3 grids x 2 pitches x every position x 4 directions x 8 lanes x V cells)
    want = sum(2 * (w + 2) * (h + 2) * 4 * 8 * v for v in (3, 5, 7) for w, h in ((8, 8), (11, 6), (16, 16)))
    assert p.stdout.startswith(f"{want} addresses"), p.stdout
