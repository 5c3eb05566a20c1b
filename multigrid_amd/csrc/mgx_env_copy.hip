// mgx_env_copy.hip -- snapshot, restore and fork of chosen envs on the device (include/mgx.h: "ENV COPY", mgx_env_copy), gfx950.
//
//   env_copy_kernel<VecT>   n (source row, destination row) pairs between two state sets, in the idiom of restart_from_pool /
//                           copy_layouts (mgx_aux.hip).  A wavefront owns `run` consecutive pairs (mgx_aux_geom.h: env_copy_geom --
//                           about 4 KiB of tile bytes; one pair once a tile is that big).  Lane l < run takes pair l: it reads the
//                           two indices, range-checks them (a bad pair is counted and skipped whole) and moves the pair's small rows
//                           itself -- rng as two 16-byte vectors, aux as one, gen_state as three, then step_count, episode, the
//                           layout marker, the running episode's two scalars and the destination's staging tags; every load before
//                           the first store.  The indices of the live pairs go to the wavefront through two LDS arrays of its own
//                           (compacted by a ballot, no barrier: LDS traffic inside one wavefront is in order); all 64 lanes then
//                           copy the cell tiles in the widest unit VecT that divides the tile size and both base addresses
//                           (env_copy_unit), the agent rows and the running returns in 8-byte units -- in rounds of kRound vectors
//                           per lane, every load of a round issued before its stores.  Tiles of 64 vectors or more go pair by pair,
//                           lanes over the vectors; smaller ones as (pair, vector) items flattened over the lanes, the pair found
//                           by recip32 (units == 1 has no 32-bit reciprocal: it branches, as copy_layouts does).
//                           No inter-wavefront traffic but the two `bad` words (mgx_env_rows.h: count_bad).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mgx_aux_geom.h"
#include "mgx_host.h"

namespace {

using namespace mgx;

struct EnvCopyArgs {
    int64_t n;
    int32_t run, units, A, stage_mode, marker_fill;      // pairs per wavefront; VecT units per tile
    uint32_t inv_units, inv_A;                           // recip32 of the units per tile / of the agents (copy_rows)
    int64_t tile_bytes;
    MgxEnvRows src, dst;
    const int64_t *src_idx, *dst_idx;
    int32_t *stage_tag, *bad;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));       // (a plain vector: HIP's uint4 class kept the rounds' arrays in memory)

constexpr int kRound = 4;               // vectors per lane in flight: loads of a round, then its stores

__device__ __forceinline__ void wave_sync() {          // LDS traffic inside ONE wavefront is in order: compiler fence only
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// rows of `units` VecT each: row l_src[j] of `src` -> row l_dst[j] of `dst`, j < m, with all 64 lanes
template <typename VecT>
__device__ __forceinline__ void copy_rows(int m, int units, uint32_t inv_units, int64_t row_bytes, const int64_t *l_src,
                                          const int64_t *l_dst, const uint8_t *src, uint8_t *dst, int lane) {
    if (units >= 64) {                                            // big rows: pair by pair, lanes over its vectors
        for (int j = 0; j < m; ++j) {
            const VecT *s = reinterpret_cast<const VecT *>(src + l_src[j] * row_bytes);
            VecT *d = reinterpret_cast<VecT *>(dst + l_dst[j] * row_bytes);
            for (int v0 = lane; v0 < units; v0 += 64 * kRound) {
                VecT r[kRound];
#pragma unroll
                for (int k = 0; k < kRound; ++k)
                    if (v0 + 64 * k < units) r[k] = s[v0 + 64 * k];
#pragma unroll
                for (int k = 0; k < kRound; ++k)
                    if (v0 + 64 * k < units) d[v0 + 64 * k] = r[k];
            }
        }
    } else {                                                      // small rows: (pair, vector) items flattened over the lanes
        const int total = m * units;                              // (< 64 * 64: recip32 is exact far beyond)
        for (int k0 = lane; k0 < total; k0 += 64 * kRound) {
            VecT r[kRound];
            VecT *d[kRound];
#pragma unroll
            for (int k = 0; k < kRound; ++k) {
                const int item = k0 + 64 * k;
                if (item < total) {
                    const int j = units == 1 ? item : (int)__umulhi((uint32_t)item, inv_units), v = item - j * units;
                    r[k] = reinterpret_cast<const VecT *>(src + l_src[j] * row_bytes)[v];
                    d[k] = reinterpret_cast<VecT *>(dst + l_dst[j] * row_bytes) + v;
                }
            }
#pragma unroll
            for (int k = 0; k < kRound; ++k)
                if (k0 + 64 * k < total) *d[k] = r[k];
        }
    }
}

// rows of `units` 8-byte words of `dst` zeroed (the running returns of a destination whose source carries none)
__device__ __forceinline__ void zero_rows(int m, int units, uint32_t inv_units, const int64_t *l_dst, uint64_t *dst, int lane) {
    const int total = m * units;
    for (int item = lane; item < total; item += 64) {
        const int j = units == 1 ? item : (int)__umulhi((uint32_t)item, inv_units), v = item - j * units;
        dst[l_dst[j] * units + v] = 0;
    }
}

template <typename VecT>
__global__ __launch_bounds__(64 * kEnvCopyWpb) void env_copy_kernel(const EnvCopyArgs a) {
    __shared__ int64_t s_src[kEnvCopyWpb][64], s_dst[kEnvCopyWpb][64];
    const RowWave w = row_wave<kEnvCopyWpb>(a.run);
    if (w.p0 >= a.n) return;
    const int lane = w.lane, wave = w.wave;
    const int64_t i = w.p0 + lane;
    int64_t s = 0, d = 0;
    bool ok = false;
    if (lane < a.run && i < a.n) {
        const bool ok_s = pick_row(a.src_idx, i, a.src.rows, s), ok_d = pick_row(a.dst_idx, i, a.dst.rows, d);
        ok = ok_s && ok_d;
        if (!ok) count_bad(a.bad, i);                                     // the PAIR is skipped whole, and counted once
    }
    if (ok) {
        // the pair's small rows: what both sets carry, every load before the first store
        const bool aux = a.src.aux && a.dst.aux, gen = a.src.gen_state && a.dst.gen_state, epi = a.src.episode && a.dst.episode;
        const bool trio = a.dst.cur_length != nullptr, trio_src = a.src.cur_length != nullptr;
        const u32x4 *rs = reinterpret_cast<const u32x4 *>(a.src.rng) + s * 2;
        const u32x4 r0 = rs[0], r1 = rs[1];
        u32x4 x = {0, 0, 0, 0}, g0 = x, g1 = x, g2 = x;
        if (aux) x = reinterpret_cast<const u32x4 *>(a.src.aux)[s];
        if (gen) {
            const u32x4 *gs = reinterpret_cast<const u32x4 *>(a.src.gen_state) + s * 3;
            g0 = gs[0]; g1 = gs[1]; g2 = gs[2];
        }
        const int32_t sc = a.src.step_count[s];
        int32_t ep = 0, mk = -1, len = 0;
        uint8_t over = 0;
        if (epi) ep = a.src.episode[s];
        if (a.dst.marker && a.src.marker && !a.marker_fill) mk = a.src.marker[s];
        if (trio && trio_src) { len = a.src.cur_length[s]; over = a.src.over[s]; }

        u32x4 *rd = reinterpret_cast<u32x4 *>(a.dst.rng) + d * 2;
        rd[0] = r0; rd[1] = r1;
        if (aux) reinterpret_cast<u32x4 *>(a.dst.aux)[d] = x;
        if (gen) {
            u32x4 *gd = reinterpret_cast<u32x4 *>(a.dst.gen_state) + d * 3;
            gd[0] = g0; gd[1] = g1; gd[2] = g2;
        }
        a.dst.step_count[d] = sc;
        if (epi) a.dst.episode[d] = ep;
        if (a.dst.marker) a.dst.marker[d] = mk;
        if (trio) { a.dst.cur_length[d] = len; a.dst.over[d] = over; }     // (no source trio: a fresh episode, nothing counted)
        if (a.stage_tag) {                                                // the destination's staging slots are void: a cache
            if (a.stage_mode == 1) {
                reinterpret_cast<u32x4 *>(a.stage_tag)[d] = u32x4{~0u, ~0u, ~0u, ~0u};
            } else if (a.stage_mode == 2) {
                a.stage_tag[d * 4 + 0] = -1;
                a.stage_tag[d * 4 + 3] = 0;
            }
        }
    }
    const uint64_t mask = __builtin_amdgcn_ballot_w64(ok);
    if (mask == 0) return;
    const int m = __builtin_popcountll(mask);
    if (ok) {
        const int pos = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        s_src[wave][pos] = s; s_dst[wave][pos] = d;
    }
    wave_sync();
    const int64_t *l_src = s_src[wave], *l_dst = s_dst[wave];
    copy_rows<VecT>(m, a.units, a.inv_units, a.tile_bytes, l_src, l_dst, reinterpret_cast<const uint8_t *>(a.src.cells),
                    reinterpret_cast<uint8_t *>(a.dst.cells), lane);
    copy_rows<uint64_t>(m, a.A, a.inv_A, (int64_t)a.A * MGX_AGENT_STRIDE, l_src, l_dst, a.src.agents, a.dst.agents, lane);   // 8-byte rows
    if (a.dst.cur_return) {
        if (a.src.cur_return)
            copy_rows<uint64_t>(m, a.A, a.inv_A, (int64_t)a.A * 8, l_src, l_dst, reinterpret_cast<const uint8_t *>(a.src.cur_return),
                                reinterpret_cast<uint8_t *>(a.dst.cur_return), lane);
        else
            zero_rows(m, a.A, a.inv_A, l_dst, reinterpret_cast<uint64_t *>(a.dst.cur_return), lane);
    }
}

// the kernel's instantiation for a copy unit of 16 / 8 / 4 / 2 / 1 bytes (mgx_aux_geom.h: env_copy_unit)
#define MGX_ENV_COPY_BY_UNIT(unit)                                                                                              \
    ((unit) == 16 ? env_copy_kernel<u32x4> : (unit) == 8 ? env_copy_kernel<uint64_t> : (unit) == 4 ? env_copy_kernel<uint32_t> \
     : (unit) == 2 ? env_copy_kernel<uint16_t> : env_copy_kernel<uint8_t>)

// a state set that is copied: every member moves, and the running trio is there whole or not at all
int check_copied(const MgxEnvRows &r, int cb) {
    const int trio = (r.cur_return != nullptr) + (r.cur_length != nullptr) + (r.over != nullptr);
    if (trio != 0 && trio != 3) return MGX_ERR_INVALID_ARGUMENT;
    return check_rows(r, ROWS_CELLS | ROWS_AGENTS | ROWS_RNG | ROWS_STEP_COUNT, ROWS_ALL, cb);
}

}  // namespace

extern "C" {

int mgx_env_copy(const MgxSpec *spec, int64_t n, const MgxEnvRows *src, const int64_t *src_idx, const MgxEnvRows *dst,
                 const int64_t *dst_idx, int32_t *stage_tag, int32_t stage_mode, int32_t marker_fill, int32_t *bad, void *stream) {
    if (check_rows_spec(spec) || n < 0 || !src || !dst) return MGX_ERR_INVALID_ARGUMENT;
    if (src->rows < 0 || dst->rows < 0 || stage_mode < 0 || stage_mode > 2) return MGX_ERR_INVALID_ARGUMENT;
    if (n == 0) return MGX_OK;
    const int cb = cell_bytes(spec->cell_bytes);
    if (check_copied(*src, cb) || check_copied(*dst, cb) || misaligned(dst_idx, 8) || misaligned(stage_tag, 16))
        return MGX_ERR_INVALID_ARGUMENT;
    if (const int rc = check_rows_n(n, src_idx, bad, kEnvCopyWpb)) return rc;
    const int tile_bytes = spec->width * spec->height * cb;
    const EnvCopyGeom g = env_copy_geom(tile_bytes, n);
    if (g.blocks > INT_MAX) return MGX_ERR_UNSUPPORTED;
    // widest copy unit that divides the tile size and both base addresses (mgx_aux_geom.h)
    const ResetUnit u = env_copy_unit(tile_bytes, reinterpret_cast<uintptr_t>(src->cells), reinterpret_cast<uintptr_t>(dst->cells));
    const EnvCopyArgs args{n, g.run, u.units, spec->num_agents, stage_mode, marker_fill, recip32((uint32_t)u.units),
                           recip32((uint32_t)spec->num_agents), tile_bytes, *src, *dst, src_idx, dst_idx, stage_tag, bad};
    hipLaunchKernelGGL(MGX_ENV_COPY_BY_UNIT(u.unit), dim3((unsigned)g.blocks), dim3(64 * kEnvCopyWpb), 0,
                       static_cast<hipStream_t>(stream), args);
    return finish_launch();
}

}  // extern "C"
