// mgx_action_mask.hip -- effective-action masks of chosen env rows on the device (include/mgx.h: "ACTION MASKS", mgx_action_mask),
// gfx950.  The rule itself -- what a set bit means, the front cell of the three cell formats, the hook state -- is mgx_action_mask.h.
//
//   action_mask_kernel<CB>  masks of n chosen rows of a state set (MgxEnvRows: a live batch or a snapshot).  Every env has a group of
//                           `group` lanes (mgx_aux_geom.h: action_mask_geom -- the smallest power of two that holds its A agents),
//                           a wavefront 64 / group consecutive envs.  Each lane of a group reads the env's index itself (one address
//                           per group: a broadcast) and range-checks it; a bad index is counted by the group's first lane and its
//                           output bytes are left alone.  Lane k < A then loads agent k's 8-byte row ONCE and works out its front
//                           position.  Whether an agent row stands there is asked across the group's lanes: A rounds of one
//                           __shfl of the packed positions, no row is read twice.  A live agent whose front position is inside
//                           the grid then makes its ONE gather -- the front cell, cb bytes at (fy * W + fx) * cb of the env's own
//                           tile; nobody else reads a cell -- and the env's 16 aux bytes (one address per group) where the env kind
//                           has a hook that matters.  Output: one byte per lane (consecutive lanes, consecutive bytes), or with
//                           MGX_MASK_EXPAND the env's 7 * A bytes in rounds of `group` consecutive bytes, byte t taking agent t / 7's
//                           mask from its lane by a __shfl.  Byte stores: the output may start at any address.  No LDS, no
//                           inter-wavefront traffic but the two `bad` words (mgx_env_rows.h: count_bad).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mgx_action_mask.h"
#include "mgx_aux_geom.h"
#include "mgx_host.h"

namespace {

using namespace mgx;

struct ActionMaskArgs {
    int64_t n, rows;
    int32_t group, group_shift;         // lanes per env = 1 << group_shift
    int32_t A, W, H, env_kind;
    int32_t allow_overlap, expand;
    int64_t tile_bytes;
    const uint8_t *cells, *agents, *aux;
    const int64_t *src_idx;
    uint8_t *mask;
    int32_t *bad;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int CB>
__global__ __launch_bounds__(64 * kMaskWpb) void action_mask_kernel(const ActionMaskArgs a) {
    const RowWave w = row_wave<kMaskWpb>(64 >> a.group_shift);
    if (w.p0 >= a.n) return;                                      // (the lanes below stay together through the shuffles)
    const int lane = w.lane, k = lane & (a.group - 1), first = lane - k;     // the agent of this lane; lane 0 of its group
    const int64_t i = w.p0 + (lane >> a.group_shift);
    int64_t s = 0;
    bool ok = false;
    if (i < a.n) ok = pick_row(a.src_idx, i, a.rows, k == 0, a.bad, s);      // (a bad index: its bytes are left alone)
    const bool mine = ok && k < a.A;
    uint64_t row = 0;
    if (mine) row = reinterpret_cast<const uint64_t *>(a.agents)[s * a.A + k];
    int fx = 0, fy = 0;
    const bool live = mine && !row_term(row);
    const bool front = mask_front(row, a.W, a.H, fx, fy) && live;  // only then is a cell read
    // presence: does any agent row of the env (terminated ones count) stand at (fx, fy)?  Positions are bytes: a front position
    // beyond 255 is nobody's.  Lanes without an agent offer a position no front can have.
    const uint32_t pos = mine ? ((uint32_t)(row >> 16) & 0xffffu) : 0xffffffffu;
    const uint32_t want = (front && fx < 256 && fy < 256) ? ((uint32_t)fx | ((uint32_t)fy << 8)) : 0xfffffffeu;
    bool present = false;
#pragma unroll 4
    for (int j = 0; j < a.A; ++j) present |= (uint32_t)__shfl((int)pos, first + j) == want;

    uint32_t bits = live ? (MASK_LEFT | MASK_RIGHT) : 0u;
    if (front) {
        const uint8_t *cellp = a.cells + s * a.tile_bytes + (int64_t)(fy * a.W + fx) * CB;
        const uint32_t cell = mask_cell(CB, cellp);
        bool stale = false, rules_hit = false;
        if (a.aux && (a.env_kind == MGX_KIND_REDBLUEDOORS || a.env_kind == MGX_KIND_RULES)) {   // (wave-uniform)
            const u32x4 v = reinterpret_cast<const u32x4 *>(a.aux)[s];
            const uint32_t ax[4] = {v.x, v.y, v.z, v.w};
            mask_hook(a.env_kind, ax, fx, fy, stale, rules_hit);
        }
        bits |= mask_front_bits(cell, row_carry(row), present, a.allow_overlap != 0, stale, rules_hit);
    }

    if (!a.expand) {
        if (mine) a.mask[i * a.A + k] = (uint8_t)bits;
        return;
    }
    const int bytes = kMaskActions * a.A;
    uint8_t *out = a.mask + i * bytes;
    for (int t0 = 0; t0 < bytes; t0 += a.group) {                 // (wave-uniform trip count: every lane takes part in the shuffle)
        const int t = t0 + k;
        const uint32_t m = (uint32_t)__shfl((int)bits, first + (mask_expand_agent(t) & (a.group - 1)));
        if (ok && t < bytes) out[t] = mask_expand_byte(m, t);
    }
}

}  // namespace

extern "C" {

int mgx_action_mask(const MgxSpec *spec, int64_t n, const MgxEnvRows *src, const int64_t *src_idx, uint32_t flags, uint8_t *mask,
                    int32_t *bad, void *stream) {
    if (check_rows_spec(spec) || n < 0 || !src) return MGX_ERR_INVALID_ARGUMENT;
    if (src->rows < 0 || (flags & ~(uint32_t)MGX_MASK_EXPAND)) return MGX_ERR_INVALID_ARGUMENT;
    if (n == 0) return MGX_OK;
    const int cb = cell_bytes(spec->cell_bytes);
    const uint32_t read = ROWS_CELLS | ROWS_AGENTS;
    if (check_rows(*src, read, read | ROWS_AUX, cb) || !mask) return MGX_ERR_INVALID_ARGUMENT;
    if (const int rc = check_rows_n(n, src_idx, bad, kMaskWpb)) return rc;
    const int64_t cells = (int64_t)spec->width * spec->height;
    if (cells > 2 * 65536) return MGX_ERR_UNSUPPORTED;            // (mgx_state_key's bound: a cell's byte offset fits an int)
    const ActionMaskGeom g = action_mask_geom(spec->num_agents, n);
    if (g.blocks > INT_MAX) return MGX_ERR_UNSUPPORTED;
    const ActionMaskArgs args{n, src->rows, g.group, log2_of(g.group), spec->num_agents, spec->width, spec->height, spec->env_kind,
                              spec->allow_agent_overlap, (int32_t)(flags & MGX_MASK_EXPAND), cells * cb,
                              reinterpret_cast<const uint8_t *>(src->cells), src->agents, src->aux, src_idx, mask, bad};
    hipLaunchKernelGGL(MGX_BY_CELL_BYTES(action_mask_kernel, cb), dim3((unsigned)g.blocks), dim3(64 * kMaskWpb), 0,
                       static_cast<hipStream_t>(stream), args);
    return finish_launch();
}

}  // extern "C"
