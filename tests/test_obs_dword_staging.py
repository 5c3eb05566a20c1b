"""CPU check of the one-step kernels' dword staging of the observation (mgx_fused_body.inc P4/P5, views of one lane pass):
P4 stages every cell as one dword (type, color, state, junk) and P5 packs 4 of them into 12 output bytes with v_perm_b32
(mgx_rules.h: obs_stage_sel, obs_pack_sel, obs_shift_sel, obs_unit).  A g++ build of those functions -- v_perm_b32 restated for the
host -- replays P4 and P5 lane by lane for every lane and round, every residue of the wave's first byte mod 4, both cell formats
and partial last waves, and checks the bytes that reach memory against the packed observation.  The GPU parity tests
(test_obs_dword_staging_gpu.py and the existing ones) run the kernels themselves."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "multigrid_amd/csrc/mgx_rules.h"
using namespace mgx;

static uint64_t rs = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)rs; }

// one wavefront: NVc views of V*V cells, rounds of R slots, its obs bytes at o0 of the step's output
static int wave(int V, int R, int NVc, int64_t o0, bool c8) {
    const int V2 = V * V, vb = V2 * 3, s = (int)(o0 & 3);
    const int units = R * V2 / 4 + 1;                               // mgx_fused_body.inc: kUnits
    std::vector<uint8_t> want((size_t)NVc * vb);                    // the observation's bytes
    std::vector<uint32_t> cells((size_t)NVc * V2);                  // P4's value of each cell (16-bit cells: from packed pairs)
    for (int v = 0; v < NVc; ++v)
        for (int p = 0; p < V2; ++p) {
            const uint32_t t = rnd() % 11, col = rnd() % 6, st = rnd() % 3, seen = rnd() % 4 != 0;
            uint32_t c;
            if (c8) {
                c = t | (col << 8) | (st << 16) | (rnd() << 24);      // the decode table's entry (byte 3: anything)
                if (!seen) c = 0;
            } else {
                // a register holds the packed cells of slots 2q (low half) and 2q+1 (high half): MgxCell = type | color << 8 | state << 12
                const uint32_t mine = t | (col << 8) | (st << 12), other = (rnd() % 11) | ((rnd() % 6) << 8) | ((rnd() % 3) << 12);
                const bool hi = v & 1;
                const uint32_t x = hi ? (other | (mine << 16)) : (mine | (other << 16));
                c = perm_b32((x >> 12) & 0x00030003u, x & 0x070f070fu, obs_stage_sel(hi));
                if (!seen) c = 0;
            }
            cells[(size_t)v * V2 + p] = c;
            const uint32_t o = seen ? (t | (col << 8) | (st << 16)) : 0u;
            for (int b = 0; b < 3; ++b) want[(size_t)v * vb + 3 * p + b] = (uint8_t)(o >> (8 * b));
        }
    // the wave's dword-aligned window of the output, with guard bytes either side
    const int G = 16;
    std::vector<uint8_t> mem(G + s + (size_t)NVc * vb + G, 0xa5);
    std::vector<uint32_t> stg(4 + R * V2 + 4);                     // LdsCarve: round_bytes + 32 (pad of 4 dwords each side)
    int bad = 0;
    for (int r0 = 0; r0 < NVc; r0 += R) {
        for (auto &w : stg) w = rnd();                              // junk: what the tile left
        for (int sl = 0; sl < R; ++sl)                              // whole rounds: padding slots store junk too
            for (int p = 0; p < V2; ++p) stg[4 + sl * V2 + p] = r0 + sl < NVc ? cells[(size_t)(r0 + sl) * V2 + p] : rnd();
        const int roff = r0 * vb, ulen = s + std::min(R * vb, (NVc - r0) * vb);
        for (int u = 0; u < units; ++u) {                           // lane u + 64 k of pass k
            const int ub = 12 * u;
            if (ub >= ulen) continue;
            if (4 + 4 * u + 3 >= (int)stg.size()) { std::printf("staging read out of range u=%d\n", u); return 1; }
            uint32_t w[3];
            obs_unit(s ? stg[4 + 4 * u - 1] : 0u, stg[4 + 4 * u], stg[4 + 4 * u + 1], stg[4 + 4 * u + 2], stg[4 + 4 * u + 3], s, w);
            const bool full = ub >= s && ub + 12 <= ulen;
            const int lo = full ? 0 : std::max(s - ub, 0), hi = full ? 12 : std::min(ulen - ub, 12);
            for (int B = lo; B < hi; ++B) mem[G + roff + ub + B] = (uint8_t)(w[B >> 2] >> (8 * (B & 3)));
        }
    }
    for (size_t i = 0; i < mem.size(); ++i) {
        const long k = (long)i - G - s;
        const bool ours = k >= 0 && k < (long)want.size();
        const uint8_t e = ours ? want[k] : 0xa5;
        if (mem[i] != e && bad++ < 4)
            std::printf("V=%d R=%d NVc=%d o0%%4=%d c8=%d: byte %ld: %02x != %02x\n", V, R, NVc, s, (int)c8, k, mem[i], e);
    }
    return bad != 0;
}

int main() {
    int fails = 0, n = 0;
    for (int c8 = 0; c8 < 2; ++c8)
        for (int V : {3, 5, 7})
            for (int R : {4, 8, 16})
                for (int A = 1; A <= 5; ++A)
                    for (int NVc = 1; NVc <= 64; ++NVc)
                        for (int64_t v0 : {0, 1, 2, 3, 4 * A, 64 * 1023 + 5, 12345}) {
                            fails += wave(V, R, NVc, v0 * V * V * 3, c8);
                            ++n;
                        }
    std::printf("%d waves, %d failed\n", n, fails);
    return fails != 0;
}
"""


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    d = tmp_path_factory.mktemp("dword_staging")
    src, exe = d / "dword_staging.cpp", d / "dword_staging"
    src.write_text(SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall",
                           f"-I{ROOT}", "-o", str(exe), str(src)])
    return str(exe)


def test_perm_b32_host_form():
    # v_perm_b32's byte selection as the kernels use it: 0-3 = lo, 4-7 = hi, 12 = zero
    code = r"""
#include <cstdio>
#include "multigrid_amd/csrc/mgx_rules.h"
int main() {
    const uint32_t hi = 0x44332211u, lo = 0x88776655u;
    int ok = mgx::perm_b32(hi, lo, 0x07060504u) == hi && mgx::perm_b32(hi, lo, 0x03020100u) == lo
             && mgx::perm_b32(hi, lo, 0x0c040100u) == 0x00116655u && mgx::perm_b32(hi, lo, 0x00070400u) == 0x55441155u;
    std::printf("%d\n", ok);
    return !ok;
}
"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "perm.cpp"), os.path.join(d, "perm")
        open(src, "w").write(code)
        subprocess.check_call(["g++", "-O2", "-std=c++17", f"-I{ROOT}", "-o", exe, src])
        assert subprocess.run([exe]).returncode == 0


def test_obs_shift_selectors():
    # stage 2 moves the packed bytes up by s: byte i of the result is byte 4 - s + i of {packed k, packed k - 1}
    code = r"""
#include <cstdio>
#include "multigrid_amd/csrc/mgx_rules.h"
int main() {
    const uint32_t want[4] = {0x07060504u, 0x06050403u, 0x05040302u, 0x04030201u};
    int ok = 1;
    for (int s = 0; s < 4; ++s) ok &= mgx::obs_shift_sel(s) == want[s];
    return !ok;
}
"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sel.cpp"), os.path.join(d, "sel")
        open(src, "w").write(code)
        subprocess.check_call(["g++", "-O2", "-std=c++17", f"-I{ROOT}", "-o", exe, src])
        assert subprocess.run([exe]).returncode == 0


def test_compaction_reproduces_packed_bytes(binary):
    p = subprocess.run([binary], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    assert " 0 failed" in p.stdout
