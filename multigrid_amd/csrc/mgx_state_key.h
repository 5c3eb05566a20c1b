// mgx_state_key.h -- the key of an env state and of an agent view (include/mgx.h: "STATE KEYS"), stated once for both compilers:
// the kernels of mgx_state_key.hip mix their words with these functions, and g++ builds the same header into the stand-alone
// program of tests/test_state_key.py, which holds `state_key_host` / `obs_key_host` to a NumPy statement of the rule.
//
// A key is the XOR of key_mix(word ^ salt) over a set of 64-bit words, word = tag << 60 | idx << 32 | payload.  Every (tag, idx)
// occurs once in a key, so no two terms cancel, and XOR leaves the order in which lanes visit the words free.
#pragma once
#include "mgx_rules.h"

namespace mgx {

enum : uint32_t { KEY_TAG_CELLS = 1, KEY_TAG_AGENTS = 2, KEY_TAG_AUX = 3, KEY_TAG_STEP = 4, KEY_TAG_RNG = 5, KEY_TAG_IMAGE = 8,
                  KEY_TAG_DIR = 9 };
constexpr uint32_t KEY_NO_CELL = 0xFFFFu;                 // the partner of the last cell of an odd grid

// splitmix64 (Steele, Lea, Flood 2014): key_mix(0) = 0xE220A8397B1DCDAF
MGX_HD uint64_t key_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
MGX_HD uint64_t key_word(uint32_t tag, uint32_t idx, uint32_t payload) {
    return ((uint64_t)tag << 60) | ((uint64_t)idx << 32) | (uint64_t)payload;
}
MGX_HD uint64_t key_term(uint32_t tag, uint32_t idx, uint32_t payload, uint64_t salt) { return key_mix(key_word(tag, idx, payload) ^ salt); }

// The canonical cell c = (type & 15) | (colour & 7) << 4 | state byte << 8 (a box's content rides in the state byte, the derived
// opaque bit is no part of it) ...
// ... of a logical cell (mgx_rules.h: type | colour << 8 | state byte << 16)
MGX_HD uint32_t key_cell_logical(uint32_t c) { return (c & 15u) | ((c >> 4) & 0x70u) | ((c >> 8) & 0xff00u); }
// ... of the three formats the grid is kept in: 16-bit cells, compact cells, byte triples
MGX_HD uint32_t key_cell16(uint32_t p) { return key_cell_logical(cell_unpack_full(p & 0xffffu)); }
// ... of two 16-bit cells at once, the halves of a dword: every field moves inside its half, so the pair costs what one cell does
MGX_HD uint32_t key_pair16(uint32_t pp) {
    return (pp & 0x000F000Fu) | ((pp >> 4) & 0x03700370u) | ((pp << 6) & 0x3C003C00u) | ((pp << 3) & 0x40004000u)
           | ((pp << 1) & 0x80008000u);
}
MGX_HD uint32_t key_cell8(uint32_t p) { return key_cell_logical(cell8_unpack(p & 0xffu)); }
// ... of four compact cells at once, the bytes of a dword: w0 = the word of bytes 0 and 1, w1 = that of bytes 2 and 3.  A code
// below 8 is its own type with state 0; the codes 8..15 look their type and state up in two 8-byte tables (v_perm_b32 by the
// code's low three bits, all four cells in one go); M = 0xFF in the bytes whose code has bit 3.
MGX_HD void key_quad8(uint32_t d, uint32_t &w0, uint32_t &w1) {
    const uint32_t sel = d & 0x07070707u;
    const uint32_t type = perm_b32(0x0A0A0A04u, 0x040A0908u, sel), state = perm_b32(0x03020102u, 0x01000000u, sel);
    const uint32_t m = (d >> 3) & 0x01010101u, M = (m << 8) - m;
    const uint32_t low = (M & type) | (~M & d & 0x0F0F0F0Fu) | (d & 0x70707070u), high = state & M;      // type | colour << 4; state
    w0 = perm_b32(high, low, 0x05010400u);
    w1 = perm_b32(high, low, 0x07030602u);
}
MGX_HD uint32_t key_cell24(uint32_t t, uint32_t col, uint32_t sb) { return (t & 15u) | ((col & 7u) << 4) | ((sb & 0xffu) << 8); }

// the word of cells 2j and 2j + 1
MGX_HD uint64_t key_cells_term(uint32_t j, uint32_t c_even, uint32_t c_odd, uint64_t salt) {
    return key_term(KEY_TAG_CELLS, j, c_even | (c_odd << 16), salt);
}

MGX_HD uint32_t key_le32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// cell p of a grid of `cb`-byte cells, canonical
MGX_HD uint32_t key_cell_at(int cb, const uint8_t *cells, int p) {
    if (cb == 1) return key_cell8(cells[p]);
    if (cb == 3) return key_cell24(cells[3 * p], cells[3 * p + 1], cells[3 * p + 2]);
    return key_cell16((uint32_t)cells[2 * p] | ((uint32_t)cells[2 * p + 1] << 8));
}

// The rule, word after word.  cells: H * W cells of `cb` bytes; agents: u8[A,8]; rng: the four PCG64 words; aux: u8[16] or NULL
// (keyed as 16 zero bytes).
inline uint64_t state_key_host(int W, int H, int A, int cb, const uint8_t *cells, const uint8_t *agents, const uint64_t *rng,
                               int32_t step_count, const uint8_t *aux, uint32_t flags, uint64_t salt) {
    const int HW = W * H;
    uint64_t key = 0;
    for (int j = 0; 2 * j < HW; ++j) {
        const uint32_t c0 = key_cell_at(cb, cells, 2 * j), c1 = 2 * j + 1 < HW ? key_cell_at(cb, cells, 2 * j + 1) : KEY_NO_CELL;
        key ^= key_cells_term((uint32_t)j, c0, c1, salt);
    }
    for (int t = 0; t < 2 * A; ++t) key ^= key_term(KEY_TAG_AGENTS, (uint32_t)t, key_le32(agents + 4 * t), salt);
    for (int t = 0; t < 4; ++t) key ^= key_term(KEY_TAG_AUX, (uint32_t)t, aux ? key_le32(aux + 4 * t) : 0u, salt);
    if (flags & MGX_KEY_STEP_COUNT) key ^= key_term(KEY_TAG_STEP, 0u, (uint32_t)step_count, salt);
    if (flags & MGX_KEY_RNG)
        for (int t = 0; t < 8; ++t) key ^= key_term(KEY_TAG_RNG, (uint32_t)t, (uint32_t)(rng[t >> 1] >> (32 * (t & 1))), salt);
    return key;
}

// one agent view: img u8[v,v,3], the little-endian u32s of its bytes (zero-padded at the tail), and the direction
inline uint64_t obs_key_host(int v, const uint8_t *img, uint8_t dir, uint64_t salt) {
    const int bytes = 3 * v * v;
    uint64_t key = key_term(KEY_TAG_DIR, 0u, dir, salt);
    for (int j = 0; 4 * j < bytes; ++j) {
        uint32_t w = 0;
        for (int b = 0; b < 4 && 4 * j + b < bytes; ++b) w |= (uint32_t)img[4 * j + b] << (8 * b);
        key ^= key_term(KEY_TAG_IMAGE, (uint32_t)j, w, salt);
    }
    return key;
}

}  // namespace mgx
