// mgx_aux_geom.h -- the host-side launch arithmetic of the streaming kernels and of the persistent hand-shake's producer kernels in
// mgx_aux.hip, in one place and without any HIP dependency: the launchers call these functions, and tests/hostshim exports them so that
// tests/test_aux_branch_census.py and tests/test_persist_branch_census.py derive which kernel paths a shape reaches from the SAME
// arithmetic (not from a Python copy of it).
#ifndef MGX_AUX_GEOM_H
#define MGX_AUX_GEOM_H

#include <stdint.h>

#include "../../include/mgx.h"

namespace mgx {

// Division by multiplication, the one form these kernels use: __umulhi(n, recip32(d)) for n / d.
// recip32(d) = ceil(2^32 / d), d >= 2.  (d == 1 is not representable -- 2^32 comes out as 0 --: the kernels branch, as copy_layouts
// does at units == 1 and the granule kernels at gpe == 1.)
inline uint32_t recip32(uint32_t d) { return (uint32_t)((((uint64_t)1 << 32) + d - 1) / d); }
// __umulhi(n, recip32(d)) == n / d for every n below this (d >= 2).  With e = recip32(d) * d - 2^32 in [0, d) the product is
// n / d + n * e / (d * 2^32): its floor is the quotient's while n * e < 2^32, and the first n = d - 1 (mod d) beyond that is wrong.
inline uint64_t recip32_exact_below(uint32_t d) {
    const uint64_t two32 = (uint64_t)1 << 32, e = (uint64_t)recip32(d) * d - two32;
    return e == 0 ? two32 : (two32 + e - 1) / e;
}

// one_hot: a workgroup takes chunks of kOhCells cells; at most 4096 workgroups, the rest by a grid-stride loop
constexpr int kOhCells = 1024;
constexpr int kOhMaxBlocks = 256 * 16;

inline int64_t one_hot_chunks(int64_t n_cells) { return (n_cells + kOhCells - 1) / kOhCells; }
inline int64_t one_hot_blocks(int64_t n_cells) {
    const int64_t chunks = one_hot_chunks(n_cells);
    return chunks < kOhMaxBlocks ? chunks : kOhMaxBlocks;
}

// full_obs: G consecutive envs per wavefront, each wavefront with its own two LDS buffers
struct FullObsGeom {
    int G;                  // envs per wavefront
    int in_buf, out_buf;    // LDS bytes of a wavefront's input / output staging (skew + over-read pad included)
    int wave_lds;           // in_buf + out_buf
    int wpb;                // wavefronts per workgroup
    int64_t nwaves, blocks;
};

// does one env fit the 64 KiB of LDS?  (cb: bytes per grid cell, 1 / 2 / 3)
inline bool full_obs_fits(int W, int H, int cb) { return (cb + 3) * W * H + 2 * 48 <= 64 * 1024; }

inline FullObsGeom full_obs_geom(int W, int H, int cb, int64_t batch) {
    FullObsGeom g;
    const int HW = W * H;
    g.G = (6 * 1024) / (HW * 3);                                      // ~10 KiB of LDS per wavefront
    if (g.G < 1) g.G = 1;
    if (g.G * HW > 65535) g.G = 65535 / HW;
    while (g.G > 1 && (batch + g.G - 1) / g.G < 4096) g.G = (g.G + 1) / 2;   // small batches: spread over the chip
    g.in_buf = (g.G * HW * cb + 15 + 16 + 15) & ~15;                  // skew + over-read pad
    g.out_buf = (g.G * HW * 3 + 15 + 16 + 15) & ~15;
    g.wave_lds = g.in_buf + g.out_buf;
    g.wpb = 4;
    while (g.wpb > 1 && g.wpb * g.wave_lds > 64 * 1024) g.wpb >>= 1;
    g.nwaves = (batch + g.G - 1) / g.G;
    g.blocks = (g.nwaves + g.wpb - 1) / g.wpb;
    return g;
}

// reset_done: the widest copy unit (16, 8, 4, 2 or 1 bytes) that divides an env's grid bytes and both base addresses
struct ResetUnit {
    int unit, units;        // bytes per copy, copies per env
};

inline ResetUnit reset_copy_unit(int env_bytes, uintptr_t grid, uintptr_t pool_grid) {
    ResetUnit r;
    r.unit = 16;
    while (r.unit > 1 && (env_bytes % r.unit || (grid & (uintptr_t)(r.unit - 1)) || (pool_grid & (uintptr_t)(r.unit - 1)))) r.unit >>= 1;
    r.units = env_bytes / r.unit;
    return r;
}

// env_copy (mgx_env_copy.hip): the same choice for a copy between two state sets whose env rows the CALLER picks.  A row sits at an
// arbitrary multiple of the tile size behind its base, so the unit has to divide the tile size and both bases -- and nothing else:
// tile_bytes % unit == 0 and base % unit == 0 make every row's address a multiple of the unit.
inline ResetUnit env_copy_unit(int tile_bytes, uintptr_t src, uintptr_t dst) { return reset_copy_unit(tile_bytes, src, dst); }

// env_copy: a wavefront owns `run` consecutive (source, destination) pairs -- as many as make up about kEnvCopyWaveBytes of tile
// bytes, at most one per lane, at least one (a tile beyond the bound is one pair per wavefront: run * tile_bytes <=
// max(kEnvCopyWaveBytes, tile_bytes)).  A launch too small to give every SIMD of the chip a wavefront halves the run until it does or
// the run is 1 (as full_obs_geom does).  Wavefront w takes the pairs [w * run, min((w + 1) * run, n)): none is left without a pair.
constexpr int kEnvCopyWaveBytes = 4096;
constexpr int kEnvCopyWpb = 4;                   // wavefronts per workgroup
constexpr int64_t kEnvCopyFillWaves = 1024;      // 256 CUs x 4 SIMDs

struct EnvCopyGeom {
    int run;                // pairs per wavefront, 1..64
    int64_t nwaves, blocks;
};

inline EnvCopyGeom env_copy_geom(int tile_bytes, int64_t n) {
    EnvCopyGeom g;
    g.run = kEnvCopyWaveBytes / (tile_bytes < 1 ? 1 : tile_bytes);
    if (g.run > 64) g.run = 64;
    if (g.run < 1) g.run = 1;
    while (g.run > 1 && (n + g.run - 1) / g.run < kEnvCopyFillWaves) g.run = (g.run + 1) / 2;
    g.nwaves = (n + g.run - 1) / g.run;
    g.blocks = (g.nwaves + kEnvCopyWpb - 1) / kEnvCopyWpb;
    return g;
}

// state_key (mgx_state_key.hip): a wavefront owns the `run` consecutive envs env_copy_geom gives it, and every env of them a GROUP of
// lanes -- the largest power of two with group * run <= 64 (one lane per env at run = 64, the whole wavefront at run = 1).  Lane k of
// a group takes the env's chunks k, k + group, ...; a chunk is what one load covers -- `unit` bytes, but at least one key word (two
// cells), which a unit below that loads in pieces: 2 * cb bytes for 1- and 2-byte cells, 6 for byte triples.
struct StateKeyGeom {
    int run, group;         // envs per wavefront; lanes per env (a power of two)
    int64_t nwaves, blocks;
};

inline StateKeyGeom state_key_geom(int tile_bytes, int64_t n) {
    const EnvCopyGeom c = env_copy_geom(tile_bytes, n);
    StateKeyGeom g;
    g.run = c.run; g.nwaves = c.nwaves; g.blocks = c.blocks;
    g.group = 64;
    while (g.group * g.run > 64) g.group >>= 1;
    return g;
}

// the load unit of the cells: the widest of 16, 8, 4, 2, 1 bytes that divides the tile size and the base address; byte triples are
// read in units of at most 2 (a key word of theirs is 6 bytes)
inline int state_key_unit(int cb, int tile_bytes, uintptr_t cells) {
    const int unit = env_copy_unit(tile_bytes, cells, cells).unit;
    return cb == 3 && unit > 2 ? 2 : unit;
}
inline int state_key_chunk_bytes(int cb, int unit) { return cb == 3 ? 6 : (unit > 2 * cb ? unit : 2 * cb); }

// obs_key: a view of 3 * v * v bytes is ceil(3 * v * v / 4) words; its lane group is the smallest power of two that leaves a lane at
// most four of them (2 lanes at v = 3, 16 at v = 7, 64 at v = 15), a wavefront takes 64 / group views
inline int obs_key_group(int view_bytes) {
    const int words = (view_bytes + 3) / 4;
    int g = 1;
    while (g < 64 && 4 * g < words) g <<= 1;
    return g;
}

// action_mask (mgx_action_mask.hip): every env a GROUP of lanes, the smallest power of two that holds its A agents (one lane per
// agent; the lanes A .. group - 1 of a group idle), a wavefront `per` = 64 / group consecutive envs.  Wavefront w takes the envs
// [w * per, min((w + 1) * per, n)): none is left without an env.
constexpr int kMaskWpb = 4;                      // wavefronts per workgroup

struct ActionMaskGeom {
    int group, per;         // lanes per env (a power of two, A <= group <= 32); envs per wavefront
    int64_t nwaves, blocks;
};

inline ActionMaskGeom action_mask_geom(int num_agents, int64_t n) {
    ActionMaskGeom g;
    g.group = 1;
    while (g.group < num_agents && g.group < 64) g.group <<= 1;
    g.per = 64 / g.group;
    g.nwaves = (n + g.per - 1) / g.per;
    g.blocks = (g.nwaves + kMaskWpb - 1) / kMaskWpb;
    return g;
}

// distance (mgx_distance.hip): every env a GROUP of lanes, the smallest power of two that holds its H grid rows (one lane per row, at
// least 4; the lanes H .. group - 1 of a group idle), a wavefront `per` = 64 / group consecutive envs.  Wavefront w takes the envs
// [w * per, min((w + 1) * per, n)): none is left without an env.  The tile is loaded and the field stored in rounds of 64 lanes:
// `wp` lanes per grid row (the smallest power of two that holds its W columns), `rpb` = 64 / wp rows per round.
constexpr int kDistWpb = 4;                      // wavefronts per workgroup

struct DistanceGeom {
    int group, per;         // lanes per env (a power of two, max(H, 4) <= group <= 64); envs per wavefront
    int wp, rpb;            // lanes per grid row of a load / store round; rows per round
    int64_t nwaves, blocks;
};

inline DistanceGeom distance_geom(int W, int H, int64_t n) {
    DistanceGeom g;
    g.group = 4;
    while (g.group < H && g.group < 64) g.group <<= 1;
    g.per = 64 / g.group;
    g.wp = 1;
    while (g.wp < W && g.wp < 64) g.wp <<= 1;
    g.rpb = 64 / g.wp;
    g.nwaves = (n + g.per - 1) / g.per;
    g.blocks = (g.nwaves + kDistWpb - 1) / kDistWpb;
    return g;
}

// persistent stepping: granules (4 action bytes each) per env and in all, and the reciprocal the producer kernels find a granule's
// env with -- g / gpe by recip32, so the batch ends where that stops being exact (recip32_exact_below: 2^30 granules at gpe = 5,
// 1 431 655 766 at gpe = 7, beyond 2^31 at every other gpe <= 8) or at 2^31 granules, whichever comes first
inline int granule_geometry(const MgxSpec *spec, int64_t batch, int &gpe, uint32_t &inv_gpe, int64_t &ng) {
    if (!spec || batch < 1 || spec->num_agents < 1 || spec->num_agents > MGX_MAX_AGENTS) return MGX_ERR_INVALID_ARGUMENT;
    gpe = (spec->num_agents + 3) / 4;
    ng = batch * gpe;
    int64_t limit = (int64_t)1 << 31;
    if (gpe > 1 && (int64_t)recip32_exact_below((uint32_t)gpe) < limit) limit = (int64_t)recip32_exact_below((uint32_t)gpe);
    if (ng >= limit) return MGX_ERR_UNSUPPORTED;
    inv_gpe = recip32((uint32_t)gpe);
    return MGX_OK;
}

// persistent_feed: kFeedThreads threads per workgroup, kFeedPre granules per thread in registers = one chunk of kFeedSlice granules;
// one workgroup per kFeedSlice granules, at most kFeedMaxWgs (why: mgx_aux.hip, above the kernel).  Workgroup i posts the granules
// [i * per_wg, min((i + 1) * per_wg, ng_all)), per_wg rounded up to an even number: no workgroup is left without granules
// (tests/test_persist_branch_census.py walks every ng_all up to 200 000).
constexpr int kFeedPre = 8, kFeedThreads = 256, kFeedSlice = kFeedPre * kFeedThreads, kFeedMaxWgs = 32;

struct FeedGeom {
    int64_t nwg, per_wg;    // workgroups, granules per workgroup (the last one: what is left)
};

inline FeedGeom feed_geometry(int64_t ng_all) {
    FeedGeom g;
    g.nwg = (ng_all + kFeedSlice - 1) / kFeedSlice;
    if (g.nwg > kFeedMaxWgs) g.nwg = kFeedMaxWgs;
    g.per_wg = ((ng_all + g.nwg - 1) / g.nwg + 1) & ~(int64_t)1;
    return g;
}

// persistent_wait (and the feed's waits): ONE workgroup of kWaitThreads threads looks at kWaitLoads flags per thread and pass
constexpr int kWaitLoads = 8, kWaitThreads = 256, kWaitPass = kWaitLoads * kWaitThreads;

}  // namespace mgx

#endif
