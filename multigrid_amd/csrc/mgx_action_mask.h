// mgx_action_mask.h -- which of an agent's actions can do anything in the state it is in (include/mgx.h: "ACTION MASKS"), stated
// once for both compilers: the kernel of mgx_action_mask.hip asks these functions, and g++ builds the same header into the
// stand-alone program of tests/test_action_mask.py, which holds `action_mask_host` to a NumPy statement of the rule and
// `mask_front_bits` to eval_agent (mgx_rules.h) over every front cell, carry, presence, overlap setting and stale flag.
//
// A mask is one byte per agent, bit k = Action k: left 0, right 1, forward 2, pickup 3, drop 4, toggle 5; bit 6 (done) and bit 7 are 0.
// A set bit says `ev.go && (ev.nrow != row || ev.writes)` of eval_agent for that action -- the action changes the agent's row or its
// front cell -- or, in a MGX_KIND_RULES env, that a declared TOGGLES_AT rule names the front cell (conservative: such a rule can end
// an episode by a toggle that changes nothing).  Nothing here is shared with eval_agent: the fused kernels compile as they did.
#pragma once
#include "mgx_rules.h"

namespace mgx {

enum : uint32_t { MASK_LEFT = 1u << ACT_LEFT, MASK_RIGHT = 1u << ACT_RIGHT, MASK_FORWARD = 1u << ACT_FORWARD,
                  MASK_PICKUP = 1u << ACT_PICKUP, MASK_DROP = 1u << ACT_DROP, MASK_TOGGLE = 1u << ACT_TOGGLE };
constexpr int kMaskActions = 7;                           // bytes per agent of the expanded form (MGX_MASK_EXPAND)

// The front cell as `BatchedMultiGridEnv.grid` shows it, in the three cell formats: type | colour << 8 | state << 16 with the masks
// of the packed formats (type & 15, colour & 7, state & 3: what state_key keeps of a byte-grid value, less a box's content -- no
// bit of the mask depends on what a box holds).
MGX_HD uint32_t mask_cell(int cb, const uint8_t *p) {
    if (cb == 1) return cell8_unpack(*p);
    if (cb == 3) return ((uint32_t)p[0] & 15u) | (((uint32_t)p[1] & 7u) << 8) | (((uint32_t)p[2] & 3u) << 16);
    return cell_unpack(load_cell16(p));
}

// The position in front of an agent row; false when it lies outside the grid (no cell is read then).
MGX_HD bool mask_front(uint64_t row, int W, int H, int &fx, int &fy) {
    const int d = row_dir(row);
    fx = row_x(row) + dir_dx(d);
    fy = row_y(row) + dir_dy(d);
    return ((unsigned)fx < (unsigned)W) & ((unsigned)fy < (unsigned)H);
}

// byte j of the env's 16 aux bytes, held as four little-endian words (a constant j after unrolling: registers, no indexing)
MGX_HD uint32_t mask_aux_byte(const uint32_t (&aux)[4], int j) { return (aux[j >> 2] >> (8 * (j & 3))) & 0xffu; }

// What the env's hook state says about the in-bounds front position (fx, fy):
//   stale      RedBlueDoors with aux[4] set: (fx, fy) is the blue door (aux[0], aux[1]), whose object is closed whatever the grid shows
//   rules_hit  MGX_KIND_RULES: a declared TOGGLES_AT rule k < aux[0] names (fx, fy), whatever its condition
MGX_HD void mask_hook(int env_kind, const uint32_t (&aux)[4], int fx, int fy, bool &stale, bool &rules_hit) {
    const uint32_t x = (uint32_t)fx, y = (uint32_t)fy, a0 = mask_aux_byte(aux, 0), a1 = mask_aux_byte(aux, 1), a4 = mask_aux_byte(aux, 4);
    stale = (env_kind == MGX_KIND_REDBLUEDOORS) & (a4 != 0) & (x == a0) & (y == a1);
    bool hit = false;
#pragma unroll
    for (int k = 0; k < MGX_MAX_RULES; ++k) {
        const uint32_t op = mask_aux_byte(aux, 1 + 5 * k), rx = mask_aux_byte(aux, 2 + 5 * k), ry = mask_aux_byte(aux, 3 + 5 * k);
        hit |= ((uint32_t)k < a0) & (op == (uint32_t)MGX_RULE_TOGGLES_AT) & (x == rx) & (y == ry);
    }
    rules_hit = (env_kind == MGX_KIND_RULES) & hit;
}

// Bits 2..5 of a live agent whose front position is inside the grid.
//   cell     the front cell (mask_cell)                  carry   row_carry of the agent's row
//   present  some agent row of the env -- terminated ones count -- has the front position
MGX_HD uint32_t mask_front_bits(uint32_t cell, uint32_t carry, bool present, bool allow_overlap, bool stale, bool rules_hit) {
    const uint32_t type = cell & 0xffu, ctype = carry & 0xffu;
    const uint32_t state = stale ? (uint32_t)S_CLOSED : cell_state(cell);   // the door OBJECT's state
    const bool door = type == T_DOOR, empty_handed = ctype == T_EMPTY;
    const bool overlap = (type == T_EMPTY) | (type == T_GOAL) | (type == T_FLOOR) | (type == T_LAVA) | (door & (state == S_OPEN));
    const bool forward = overlap & (allow_overlap | !present);
    const bool pickup = empty_handed & ((type == T_KEY) | (type == T_BALL) | (type == T_BOX));
    const bool drop = !empty_handed & (type == T_EMPTY) & !present;
    const bool has_key = (ctype == T_KEY) & (((carry >> 8) & 0xffu) == ((cell >> 8) & 0xffu));
    const bool toggle = (type == T_BOX) | (door & ((state != S_LOCKED) | has_key)) | stale | rules_hit;
    return (forward ? MASK_FORWARD : 0u) | (pickup ? MASK_PICKUP : 0u) | (drop ? MASK_DROP : 0u) | (toggle ? MASK_TOGGLE : 0u);
}

// byte t < 7 * A of an env's expanded masks u8[A,7]: bit t % 7 of agent t / 7
MGX_HD int mask_expand_agent(int t) { return t / kMaskActions; }
MGX_HD uint8_t mask_expand_byte(uint32_t mask, int t) { return (uint8_t)((mask >> (t % kMaskActions)) & 1u); }

// The rule, agent after agent, for one env.  cells: H * W cells of `cb` bytes; agents: u8[A,8]; aux: u8[16] or NULL; mask: u8[A].
inline void action_mask_host(const MgxSpec &spec, int cb, const uint8_t *cells, const uint8_t *agents, const uint8_t *aux, uint8_t *mask) {
    const int A = spec.num_agents, W = spec.width, H = spec.height;
    uint32_t ax[4] = {0, 0, 0, 0};
    for (int j = 0; aux && j < 16; ++j) ax[j >> 2] |= (uint32_t)aux[j] << (8 * (j & 3));
    for (int a = 0; a < A; ++a) {
        uint64_t row = 0;
        for (int b = 0; b < 8; ++b) row |= (uint64_t)agents[8 * a + b] << (8 * b);
        if (row_term(row)) { mask[a] = 0; continue; }
        uint32_t m = MASK_LEFT | MASK_RIGHT;
        int fx, fy;
        if (mask_front(row, W, H, fx, fy)) {
            bool present = false;
            for (int o = 0; o < A; ++o) present |= agents[8 * o + AG_X] == fx && agents[8 * o + AG_Y] == fy;
            bool stale = false, rules_hit = false;
            if (aux) mask_hook(spec.env_kind, ax, fx, fy, stale, rules_hit);
            m |= mask_front_bits(mask_cell(cb, cells + ((size_t)fy * W + fx) * cb), row_carry(row), present, spec.allow_agent_overlap != 0,
                                 stale, rules_hit);
        }
        mask[a] = (uint8_t)m;
    }
}

}  // namespace mgx
