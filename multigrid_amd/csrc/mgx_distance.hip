// mgx_distance.hip -- walking-distance fields of chosen env rows on the device (include/mgx.h: "DISTANCE FIELDS", mgx_distance),
// gfx950.  The rule itself -- which cells a walk enters, which cells a query names -- is mgx_distance.h.
//
//   distance_kernel<CB>  a wavefront-wide, bit-parallel breadth-first flood over n chosen rows of a state set (MgxEnvRows: a live
//                        batch or a snapshot).  Every env has a group of `group` lanes (mgx_aux_geom.h: distance_geom -- the smallest
//                        power of two >= max(H, 4)), a wavefront 64 / group consecutive envs.  Lane r of a group OWNS grid row r as
//                        64-bit words, bit x = column x: `pass`, `vis` (the cells of all levels so far), the frontier, and the
//                        distance in kDistPlanes bit-planes.  Bits at columns >= W and the words of lanes >= H are zero in `pass` and
//                        in the sources, so nothing wraps at W == 64 and nothing leaks at W < 64.
//     load     the tile is read ONCE, in rounds of 64 consecutive lanes: `wp` lanes per grid row (the smallest power of two >= W),
//              64 / wp rows per round, consecutive cells at consecutive lanes.  Every lane classifies its cell; two __ballot give the
//              round's rows of `pass` and of the type / colour sources, and the lane that owns a row keeps its piece.  Agent and
//              point sources are OR-ed in by the owning lane (one address per group: a broadcast load).
//     levels   new = ((f << 1) | (f >> 1) | f_above | f_below) & pass & ~vis, the neighbouring rows' frontier words by one __shfl
//              each (zero at the group's first and last row); the level number L is wave-uniform, so plane[k] |= new happens under
//              a scalar branch for the set bits k of L.  The loop ends when no lane of the wavefront found a new cell: the trip count
//              is the deepest env's; it can never exceed H * W < 4096, which also bounds the loop.
//     field    the rounds of the load again: a lane fetches the words of the row it stores by __shfl -- only the planes the deepest
//              level of the wavefront reached -- assembles its cell's distance and stores one i16: consecutive lanes, consecutive
//              addresses, any 2-byte alignment.
//     agents   lane a < A of a group reads agent row a, fetches the words of row y and takes bit x; in rounds of `group` agents
//              when there are more agents than lanes.
//   No LDS, no inter-wavefront traffic but the two `bad` words (mgx_env_rows.h: count_bad).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mgx_aux_geom.h"
#include "mgx_distance.h"
#include "mgx_host.h"

namespace {

using namespace mgx;

struct DistanceArgs {
    int64_t n, rows;
    int32_t group, group_shift, wp_shift;   // lanes per env = 1 << group_shift; lanes per grid row of a round = 1 << wp_shift
    int32_t A, W, H;
    uint32_t type_mask, colour_mask, agent_mask, flags;
    int32_t num_points;
    int64_t tile_bytes;
    const uint8_t *cells, *agents;
    const int64_t *src_idx;
    const int16_t *points;
    int16_t *field, *agent_dist;
    int32_t *bad;
};

__device__ __forceinline__ uint64_t lane_word(uint64_t v, int src_lane) { return (uint64_t)__shfl((unsigned long long)v, src_lane); }

// the distance of column x of a row whose words sit at `src_lane`: the planes below `nplanes` (wave-uniform), -1 where `vis` is clear
__device__ __forceinline__ int16_t assemble(const uint64_t vis, const uint64_t (&plane)[kDistPlanes], int nplanes, int src_lane, int x) {
    const uint64_t v = lane_word(vis, src_lane);
    uint32_t d = 0;
#pragma unroll
    for (int k = 0; k < kDistPlanes; ++k)
        if (k < nplanes) d |= (uint32_t)((lane_word(plane[k], src_lane) >> x) & 1u) << k;
    return ((v >> x) & 1u) ? (int16_t)d : (int16_t)-1;
}

template <int CB>
__global__ __launch_bounds__(64 * kDistWpb) void distance_kernel(const DistanceArgs a) {
    const int per = 64 >> a.group_shift;
    const RowWave w = row_wave<kDistWpb>(per);
    if (w.p0 >= a.n) return;                                      // (the lanes below stay together through the shuffles)
    const int lane = w.lane;
    const int64_t p0 = w.p0;
    const int W = a.W, H = a.H, A = a.A;
    const int r = lane & (a.group - 1), first = lane - r;         // the grid row of this lane; lane 0 of its group
    const int mine = lane >> a.group_shift;                       // the env of this lane, within the wavefront
    const int64_t i = p0 + mine;
    int64_t s = 0;
    bool ok = false;
    if (i < a.n) ok = pick_row(a.src_idx, i, a.rows, r == 0, a.bad, s);      // (a bad index: its output rows are left alone)
    const uint64_t okmask = __ballot(ok);                         // bit e << group_shift: env e of the wavefront has a row to read

    // ---- load: 64 / wp rows per round; lane (ly, lx) of a round classifies cell (y0 + ly, lx)
    const int rpb = 64 >> a.wp_shift;
    const int lx = lane & ((1 << a.wp_shift) - 1), ly = lane >> a.wp_shift;
    const uint64_t piece = a.wp_shift == 6 ? ~0ull : ((1ull << (1 << a.wp_shift)) - 1ull);
    uint64_t pass = 0, vis = 0;
    for (int e = 0; e < per; ++e) {                               // (wave-uniform trip counts and branches: every lane votes)
        if (!((okmask >> (e << a.group_shift)) & 1ull)) continue;
        const int64_t se = (int64_t)lane_word((uint64_t)s, e << a.group_shift);
        const uint8_t *tile = a.cells + se * a.tile_bytes;
        for (int y0 = 0; y0 < H; y0 += rpb) {
            const int y = y0 + ly;
            const bool in = (lx < W) & (y < H);
            uint32_t cell = 0;
            if (in) cell = mask_cell(CB, tile + (y * W + lx) * CB);
            const uint64_t mp = __ballot(in && dist_passable(cell, a.flags));
            const uint64_t ms = __ballot(in && dist_source(cell, a.type_mask, a.colour_mask));
            const int j = r - y0;
            if (mine == e && j >= 0 && j < rpb) {
                pass = (mp >> (j << a.wp_shift)) & piece;
                vis = (ms >> (j << a.wp_shift)) & piece;
            }
        }
    }
    // agent and point sources, by the lane that owns their row
    const bool row_ok = ok && r < H;
    const uint64_t *rows64 = reinterpret_cast<const uint64_t *>(a.agents);
    for (uint32_t am = A >= 32 ? a.agent_mask : (a.agent_mask & ((1u << A) - 1u)); am; am &= am - 1u) {
        const int k = __builtin_ctz(am);
        if (row_ok) {
            const uint64_t row = rows64[s * A + k];
            const int x = row_x(row);
            if (row_y(row) == r && x < W) vis |= 1ull << x;
        }
    }
    for (int k = 0; k < a.num_points; ++k) {
        if (row_ok) {
            const int16_t *pt = a.points + (i * a.num_points + k) * 2;
            const int x = pt[0];
            if (pt[1] == r && x >= 0 && x < W) vis |= 1ull << x;
        }
    }

    // ---- levels
    uint64_t plane[kDistPlanes];
#pragma unroll
    for (int k = 0; k < kDistPlanes; ++k) plane[k] = 0;
    uint64_t f = vis;
    int L = 1;
    for (; L < kDistMaxSide * kDistMaxSide; ++L) {
        uint64_t above = lane_word(f, (lane - 1) & 63), below = lane_word(f, (lane + 1) & 63);
        if (r == 0) above = 0;                                    // (the neighbouring group's last / first row)
        if (r == a.group - 1) below = 0;
        const uint64_t fresh = ((f << 1) | (f >> 1) | above | below) & pass & ~vis;
        if (__ballot(fresh != 0) == 0) break;
        vis |= fresh;
#pragma unroll
        for (int k = 0; k < kDistPlanes; ++k)
            if ((L >> k) & 1) plane[k] |= fresh;                  // (a scalar branch: L is the loop's counter)
        f = fresh;
    }
    const int top = __builtin_amdgcn_readfirstlane(L - 1);       // the deepest level of the wavefront
    const int nplanes = top ? 32 - __builtin_clz((unsigned)top) : 0;

    // ---- the field: the rounds of the load, lane (ly, lx) stores cell (y0 + ly, lx)
    if (a.field) {
        for (int e = 0; e < per; ++e) {
            if (!((okmask >> (e << a.group_shift)) & 1ull)) continue;
            int16_t *out = a.field + (p0 + e) * (int64_t)(H * W);
            for (int y0 = 0; y0 < H; y0 += rpb) {
                const int y = y0 + ly;
                const int16_t d = assemble(vis, plane, nplanes, (e << a.group_shift) + (y & (a.group - 1)), lx);
                if ((lx < W) & (y < H)) out[y * W + lx] = d;
            }
        }
    }
    // ---- the agents: lane k of a group answers agent t0 + k
    if (a.agent_dist) {
        for (int t0 = 0; t0 < A; t0 += a.group) {                 // (wave-uniform trip count: every lane takes part in the shuffles)
            const int k = t0 + r;
            const bool have = ok && k < A;
            uint64_t row = 0;
            if (have) row = rows64[s * A + k];
            const int x = row_x(row), y = row_y(row);
            const int16_t d = assemble(vis, plane, nplanes, first + (y & (a.group - 1)), x & 63);
            if (have) a.agent_dist[i * A + k] = ((x < W) & (y < H)) ? d : (int16_t)-1;
        }
    }
}

}  // namespace

extern "C" {

int mgx_distance(const MgxSpec *spec, int64_t n, const MgxEnvRows *src, const int64_t *src_idx, const MgxDistance *q, int16_t *field,
                 int16_t *agent_dist, int32_t *bad, void *stream) {
    if (check_rows_spec(spec) || n < 0 || !src) return MGX_ERR_INVALID_ARGUMENT;
    if (src->rows < 0 || !q || (q->flags & ~kDistFlags) || q->num_points < 0) return MGX_ERR_INVALID_ARGUMENT;
    if (n == 0) return MGX_OK;
    const int cb = cell_bytes(spec->cell_bytes);
    const uint32_t read = ROWS_CELLS | ROWS_AGENTS;
    if (check_rows(*src, read, read, cb) || (!field && !agent_dist) || (q->num_points > 0 && !q->points)) return MGX_ERR_INVALID_ARGUMENT;
    if (misaligned(field, 2) || misaligned(agent_dist, 2) || misaligned(q->points, 2)) return MGX_ERR_INVALID_ARGUMENT;
    if (const int rc = check_rows_n(n, src_idx, bad, kDistWpb)) return rc;
    if (spec->width > kDistMaxSide || spec->height > kDistMaxSide) return MGX_ERR_UNSUPPORTED;   // (a lane per row, a bit per column)
    const DistanceGeom g = distance_geom(spec->width, spec->height, n);
    if (g.blocks > INT_MAX) return MGX_ERR_UNSUPPORTED;
    const DistanceArgs args{n, src->rows, g.group, log2_of(g.group), log2_of(g.wp), spec->num_agents, spec->width, spec->height,
                            q->type_mask, q->colour_mask, q->agent_mask, q->flags, q->num_points,
                            (int64_t)spec->width * spec->height * cb, reinterpret_cast<const uint8_t *>(src->cells), src->agents, src_idx,
                            q->num_points > 0 ? q->points : nullptr, field, agent_dist, bad};
    hipLaunchKernelGGL(MGX_BY_CELL_BYTES(distance_kernel, cb), dim3((unsigned)g.blocks), dim3(64 * kDistWpb), 0,
                       static_cast<hipStream_t>(stream), args);
    return finish_launch();
}

}  // extern "C"
