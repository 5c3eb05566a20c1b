// view_shim.cpp -- TEST INFRASTRUCTURE.  The g++ build of the view frames' key rule (multigrid_amd/csrc/mgx_render.h:
// render_view_key, include/mgx.h "VIEW FRAMES") for tests/test_view_frames_host.py, two ways from this one file:
//   * a shared library: shim_view_keys evaluates the header's rule over arrays, for the comparison with the NumPy composer;
//   * a program (its own main; built with -fsanitize=address,undefined and run directly): every cell (type, colour, state) in
//     256^3 x the 4 viewer directions x {the viewer's own cell, another cell} x highlight {off, on}, the header's key against
//     the table-driven restatement below, and every key below 2 500.  Prints "checked <n> mismatches <m> out_of_range <r>".
#include <cstdint>
#include <cstdio>

#include "../../multigrid_amd/csrc/mgx_render.h"

extern "C" {

// cells u8[n, 3]; own, dir, colour u8[n]; out i32[n]
void shim_view_keys(int64_t n, const uint8_t *cells, const uint8_t *own, const uint8_t *dir, const uint8_t *colour, int highlight,
                    int32_t *out) {
    for (int64_t k = 0; k < n; k++)
        out[k] = mgx::render_view_key(cells[3 * k], cells[3 * k + 1], cells[3 * k + 2], own[k] != 0, dir[k], colour[k], highlight != 0);
}

}

namespace {

// The rule restated from tables.  First appearance of every type (include/mgx.h: 0 empty | 1-6 wall and goal | 7-12 floor |
// 13-30 door, 3 * colour + state | 31-36 key | 37-42 ball | 43-48 box | 49 lava); -1: the type draws no object.
//                         unseen empty wall floor door key ball box goal lava agent
const int kFirst[11] = {   -1,    -1,   1,   7,    13,  31, 37,  43, 1,   49,  -1 };
const int kPerColour[11] = { 0,    0,   1,   1,    3,   1,  1,   1,  1,   0,   0 };

int table_key(int t, int c, int s, bool own, int dir, int own_colour, bool highlight) {
    int appearance = 0;
    if (t <= 10 && kFirst[t] >= 0) {
        if (t == 9)
            appearance = 49;                                                     // lava ignores its colour
        else if (c <= 5) {
            const int state = t == 4 ? (s & 3) : 0;                              // only a door's state is drawn
            appearance = (t == 4 && state == 3) ? 0 : kFirst[t] + kPerColour[t] * c + state;
        }
    }
    int overlay = 0;
    if (own) {
        if (own_colour <= 5) overlay = 1 + 4 * own_colour + 3;                   // the viewer faces up
    } else if (t == 10 && c <= 5) {
        const int rel[4] = {3, 0, 1, 2};                                         // world direction minus the viewer's, mod 4 -> drawn
        overlay = 1 + 4 * c + rel[((s & 3) - (dir & 3) + 4) % 4];
    }
    const int hl = highlight && t != 0 ? 1 : 0;
    return (appearance * 25 + overlay) * 2 + hl;
}

}  // namespace

int main() {
    long long checked = 0, mismatches = 0, out_of_range = 0;
    for (int t = 0; t < 256; t++)
        for (int c = 0; c < 256; c++)
            for (int s = 0; s < 256; s++)
                for (int dir = 0; dir < 4; dir++)
                    for (int own = 0; own < 2; own++) {
                        const int colour = (t + 3 * c + 5 * s + dir) & 7;         // the viewer's colour: 0..7 (6, 7: no overlay)
                        for (int hl = 0; hl < 2; hl++) {
                            const int key = mgx::render_view_key((uint32_t)t, (uint32_t)c, (uint32_t)s, own != 0, (uint32_t)dir,
                                                                 (uint32_t)colour, hl != 0);
                            checked++;
                            mismatches += key != table_key(t, c, s, own != 0, dir, colour, hl != 0);
                            out_of_range += key < 0 || key >= mgx::RENDER_KEYS;
                        }
                    }
    // the bytes the loop above does not reach: every viewer colour and every direction byte, on a few cells
    const int cells[6][3] = {{0, 0, 0}, {1, 0, 0}, {10, 2, 1}, {10, 7, 255}, {5, 4, 0}, {255, 255, 255}};
    for (auto &cell : cells)
        for (int dir = 0; dir < 256; dir++)
            for (int colour = 0; colour < 256; colour++)
                for (int own = 0; own < 2; own++)
                    for (int hl = 0; hl < 2; hl++) {
                        const int key = mgx::render_view_key((uint32_t)cell[0], (uint32_t)cell[1], (uint32_t)cell[2], own != 0,
                                                             (uint32_t)dir, (uint32_t)colour, hl != 0);
                        checked++;
                        mismatches += key != table_key(cell[0], cell[1], cell[2], own != 0, dir, colour, hl != 0);
                        out_of_range += key < 0 || key >= mgx::RENDER_KEYS;
                    }
    printf("checked %lld mismatches %lld out_of_range %lld\n", checked, mismatches, out_of_range);
    return mismatches || out_of_range ? 1 : 0;
}
