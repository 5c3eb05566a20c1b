// mgx_env_rows.h -- the conventions of a STATE SET (include/mgx.h: MgxEnvRows -- a live batch or a snapshot) and of the kernels that
// read chosen rows of one, stated once: mgx_env_copy.hip, mgx_state_key.hip, mgx_action_mask.hip and mgx_distance.hip check their
// arguments, split their launch over wavefronts, pick their rows and count the bad ones with what stands here.  The host part has no
// HIP dependency (g++ includes it as it does mgx_aux_geom.h); the device part is under __HIPCC__.
#ifndef MGX_ENV_ROWS_H
#define MGX_ENV_ROWS_H

#include <limits.h>
#include <stdint.h>

#include "../../include/mgx.h"

namespace mgx {

inline bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }     // (NULL is aligned)

// bytes per cell of MgxSpec.cell_bytes (0 and 2: the 16-bit cells)
inline int cell_bytes(int spec_cell_bytes) { return spec_cell_bytes == 1 ? 1 : (spec_cell_bytes == 3 ? 3 : MGX_CELL_BYTES); }

inline int log2_of(int pow2) {
    int s = 0;
    while ((1 << s) < pow2) ++s;
    return s;
}

// the spec of a row query: what the launchers read of it
inline int check_rows_spec(const MgxSpec *spec) {
    if (!spec || spec->num_agents < 1 || spec->num_agents > MGX_MAX_AGENTS || spec->width < 1 || spec->height < 1
        || spec->cell_bytes < 0 || spec->cell_bytes > 3)
        return MGX_ERR_INVALID_ARGUMENT;
    return MGX_OK;
}

// the members of a state set as bits, in the order of struct MgxEnvRows
enum : uint32_t {
    ROWS_CELLS = 1u << 0, ROWS_AGENTS = 1u << 1, ROWS_RNG = 1u << 2, ROWS_STEP_COUNT = 1u << 3, ROWS_AUX = 1u << 4, ROWS_MARKER = 1u << 5,
    ROWS_EPISODE = 1u << 6, ROWS_GEN_STATE = 1u << 7, ROWS_CUR_RETURN = 1u << 8, ROWS_CUR_LENGTH = 1u << 9, ROWS_OVER = 1u << 10,
    ROWS_ALL = (1u << 11) - 1u
};

// a state set as a call uses it: the members of `need` are there, the members of `aligned` sit where the kernel's accesses want them
// -- 16 bytes for what is read as 16-byte vectors (rng, aux, gen_state), 8 for the 8-byte rows (agents, cur_return), 4 for i32, 2 for
// 16-bit cells (cb: cell_bytes() of the spec).  A member in neither is not looked at.
inline int check_rows(const MgxEnvRows &r, uint32_t need, uint32_t aligned, int cb) {
    const struct { const void *p; uintptr_t align; } m[] = {
        {r.cells, (uintptr_t)(cb == 2 ? 2 : 1)}, {r.agents, 8}, {r.rng, 16}, {r.step_count, 4}, {r.aux, 16}, {r.marker, 4},
        {r.episode, 4}, {r.gen_state, 16}, {r.cur_return, 8}, {r.cur_length, 4}, {r.over, 1}};
    for (int k = 0; k < 11; ++k)
        if ((((need >> k) & 1u) && !m[k].p) || (((aligned >> k) & 1u) && misaligned(m[k].p, m[k].align))) return MGX_ERR_INVALID_ARGUMENT;
    return MGX_OK;
}

// the items of a launch of `wpb` wavefronts per workgroup: an index array of 8-byte words, `bad` of 4-byte ones, and no more items
// than INT_MAX workgroups can hold at one item per lane
inline int check_rows_n(int64_t n, const int64_t *idx, const int32_t *bad, int wpb) {
    if (misaligned(idx, 8) || misaligned(bad, 4)) return MGX_ERR_INVALID_ARGUMENT;
    return n > (int64_t)INT_MAX * 64 * wpb ? MGX_ERR_UNSUPPORTED : MGX_OK;
}

}  // namespace mgx

#ifdef __HIPCC__

// a kernel template's instantiation for the cell format `cb` (cell_bytes())
#define MGX_BY_CELL_BYTES(kernel, cb) ((cb) == 1 ? kernel<1> : ((cb) == 3 ? kernel<3> : kernel<2>))

namespace mgx {

// Wavefront `wave` of a workgroup of WPB wavefronts owns the `per` consecutive items of the launch from `p0`; a kernel returns where
// p0 >= n -- a wave-uniform branch, so the lanes of a wavefront that goes on stay together through its shuffles and ballots.
struct RowWave {
    int lane, wave;
    int64_t p0;
};

template <int WPB>
__device__ __forceinline__ RowWave row_wave(int per) {
    RowWave w;
    w.lane = threadIdx.x & 63;
    w.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    w.p0 = ((int64_t)blockIdx.x * WPB + w.wave) * per;
    return w;
}

// item i's row of a state set of `rows` rows: idx[i], or i without an index array.  False: the index names no row.
__device__ __forceinline__ bool pick_row(const int64_t *idx, int64_t i, int64_t rows, int64_t &s) {
    s = idx ? idx[i] : i;
    return s >= 0 && s < rows;
}

// THE `bad` WORDS (i32[2], or NULL: nothing is counted): an item whose index names no row is skipped whole -- no byte of its output
// is written -- and counted once, bad[0] += 1, bad[1] = min(bad[1], i): the convention of the step's `err` words, which start at
// {0, INT32_MAX}; an item beyond INT32_MAX counts as INT32_MAX.  Plain atomics: the only traffic between wavefronts.
__device__ __forceinline__ void count_bad(int32_t *bad, int64_t i) {
    if (bad) {
        atomicAdd(bad, 1);
        atomicMin(bad + 1, (int32_t)(i < INT_MAX ? i : INT_MAX));
    }
}

// pick_row for a group of lanes that share item i: its lane with `first` set counts a bad index
__device__ __forceinline__ bool pick_row(const int64_t *idx, int64_t i, int64_t rows, bool first, int32_t *bad, int64_t &s) {
    const bool ok = pick_row(idx, i, rows, s);
    if (!ok && first) count_bad(bad, i);
    return ok;
}

}  // namespace mgx

#endif  // __HIPCC__

#endif
