// mgx_distance.h -- walking distances over an env's grid (include/mgx.h: "DISTANCE FIELDS"), stated once for both compilers: the
// kernel of mgx_distance.hip asks `dist_passable` / `dist_source` of every cell it loads, and g++ builds the same header into the
// stand-alone program of tests/test_distance.py, which holds them and `dist_reference` -- a plain queue flood -- to a NumPy statement
// of the rule, and base passability to the `forward` bit of mask_front_bits (mgx_action_mask.h) with nobody present.
//
// A cell is what mask_cell (mgx_action_mask.h) gives: type | colour << 8 | state << 16 after the masks of the packed formats.
// Distances count moves; turns are free.  Nothing here is shared with the step kernels: they compile as they did.
#pragma once
#include "mgx_action_mask.h"

namespace mgx {

constexpr uint32_t kDistFlags = MGX_DIST_THROUGH_CLOSED | MGX_DIST_THROUGH_LOCKED | MGX_DIST_THROUGH_OBJECTS | MGX_DIST_AVOID_LAVA;
constexpr int kDistMaxSide = 64;                          // one lane per grid row, one bit of a 64-bit word per column
constexpr int kDistPlanes = 12;                           // every distance is < 64 * 64 = 2^12

// Can a walk enter this cell?  (base: what `forward` enters when nobody stands there)
MGX_HD bool dist_passable(uint32_t cell, uint32_t flags) {
    const uint32_t type = cell & 0xffu, state = cell_state(cell);
    const bool door = type == T_DOOR;
    const bool base = (type == T_EMPTY) | (type == T_FLOOR) | (type == T_GOAL) | ((type == T_LAVA) & !(flags & MGX_DIST_AVOID_LAVA))
                    | (door & (state == S_OPEN));
    const bool closed = door & (state == S_CLOSED) & ((flags & MGX_DIST_THROUGH_CLOSED) != 0);
    const bool locked = door & (state == S_LOCKED) & ((flags & MGX_DIST_THROUGH_LOCKED) != 0);
    const bool object = ((type == T_KEY) | (type == T_BALL) | (type == T_BOX)) & ((flags & MGX_DIST_THROUGH_OBJECTS) != 0);
    return base | closed | locked | object;
}

// Do the type / colour masks of a query name this cell?
MGX_HD bool dist_source(uint32_t cell, uint32_t type_mask, uint32_t colour_mask) {
    const uint32_t type = cell & 15u, colour = (cell >> 8) & 7u;
    return ((type_mask >> type) & 1u) & ((colour_mask >> colour) & 1u);
}

// The field of one env, cell after cell through a queue.  cells: H * W decoded cells (mask_cell); agents: u8[A,8]; points: i16[P,2]
// of this OUTPUT row, or NULL; field: i16[H * W], may be NULL; agent_dist: i16[A], may be NULL; queue: H * W ints of scratch.
inline void dist_reference(int W, int H, int A, const uint32_t *cells, const uint8_t *agents, const MgxDistance &q, const int16_t *points,
                           int16_t *field, int16_t *agent_dist, int16_t *d, int32_t *queue) {
    const int HW = W * H;
    int head = 0, tail = 0;
    for (int p = 0; p < HW; ++p) d[p] = -1;
    auto seed = [&](int x, int y) {
        if (x < 0 || x >= W || y < 0 || y >= H || d[y * W + x] == 0) return;
        d[y * W + x] = 0;
        queue[tail++] = y * W + x;
    };
    for (int p = 0; p < HW; ++p)
        if (dist_source(cells[p], q.type_mask, q.colour_mask)) seed(p % W, p / W);
    for (int a = 0; a < A; ++a)
        if ((q.agent_mask >> a) & 1u) seed(agents[8 * a + AG_X], agents[8 * a + AG_Y]);
    for (int k = 0; points && k < q.num_points; ++k) seed(points[2 * k], points[2 * k + 1]);
    while (head < tail) {
        const int p = queue[head++], x = p % W, y = p / W;
        const int nx[4] = {x + 1, x - 1, x, x}, ny[4] = {y, y, y + 1, y - 1};
        for (int j = 0; j < 4; ++j) {
            if (nx[j] < 0 || nx[j] >= W || ny[j] < 0 || ny[j] >= H) continue;
            const int o = ny[j] * W + nx[j];
            if (d[o] >= 0 || !dist_passable(cells[o], q.flags)) continue;
            d[o] = (int16_t)(d[p] + 1);
            queue[tail++] = o;
        }
    }
    for (int p = 0; field && p < HW; ++p) field[p] = d[p];
    for (int a = 0; agent_dist && a < A; ++a) {
        const int x = agents[8 * a + AG_X], y = agents[8 * a + AG_Y];
        agent_dist[a] = (x < W && y < H) ? d[y * W + x] : (int16_t)-1;
    }
}

}  // namespace mgx
