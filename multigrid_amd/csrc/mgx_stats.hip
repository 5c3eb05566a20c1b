// mgx_stats.hip -- episode accounting on the device (include/mgx.h: mgx_episode_stats / mgx_episode_restart), gfx950.
//
//   episode_stats_kernel    the rule of include/mgx.h over the outputs of `steps` consecutive steps.  A wavefront owns G = 64 / A whole
//                           envs: lane g * A + a is agent a of its env g (lanes >= G * A idle), so the wavefront's rewards of one step
//                           are 8 contiguous bytes per lane and its terminated bytes one per lane.  "Every agent terminated" is one
//                           ballot of those bytes and a shift-and-mask per env; "any return > 0" of a closing env likewise.  No LDS, no
//                           barrier, no atomics: every env's arithmetic is its own lanes', in step order -- bit for bit a sequential
//                           model.  The running episode (cur_return, cur_length, over) stays in registers across the step loop; every
//                           lane of an env keeps its own copy of the env's two scalars (the flag bytes are one address per env: the
//                           lanes' loads coalesce), lane a == 0 stores them.  The inputs of step t + 1 are requested before step t is
//                           applied (they do not depend on the state).  Totals, last_* and counts are touched by a closing (or
//                           aborting) env only.
//   episode_restart_kernel  the restart clause alone, one lane per env; a wavefront nobody is chosen in ends after one byte load per
//                           lane (as reset_generate_select_kernel does).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mgx_host.h"

namespace {

using namespace mgx;

struct StatsArgs {
    int64_t batch;
    int32_t A, G, steps, restart;
    const double *reward;
    const uint8_t *terminated, *truncated, *was_reset;
    MgxEpisodeStats st;
    MgxEpisodeTrace tr;
};

constexpr int kStatsWaves = 4;          // wavefronts per workgroup

__global__ __launch_bounds__(64 * kStatsWaves) void episode_stats_kernel(const StatsArgs s) {
    const int lane = threadIdx.x & 63;
    const int A = s.A;
    const int g = lane / A, a = lane - g * A;
    const int64_t wave = (int64_t)blockIdx.x * kStatsWaves + (threadIdx.x >> 6);
    const int64_t b = wave * s.G + g;
    const bool live = g < s.G && b < s.batch;
    const bool lead = live && a == 0;
    const int64_t B = s.batch;
    const int64_t ba = b * A + a;                                         // this lane's (env, agent)
    const int64_t BA = B * A;
    const int sh = g * A;                                                 // the env's lanes in a ballot: bits [sh, sh + A)
    const uint64_t ones = (A >= 64 ? 0 : (1ull << A)) - 1ull;
    const int mode = s.was_reset ? s.restart : MGX_RESTART_NONE;

    // Every lane loads, from valid addresses: an idle lane reads env 0 (its values are never used), a call without restarts reads
    // `truncated` in place of `was_reset` (never looked at).  No branch around a load, so the first step's inputs and the state
    // are ONE round of requests, and the loop can wait for step t's inputs while those of step t + 1 are still on their way.
    const int64_t bs = live ? b : 0, bas = live ? ba : 0;
    const uint8_t *const wr_p = mode != MGX_RESTART_NONE ? s.was_reset : s.truncated;
    double r = s.reward[bas];
    uint32_t te = s.terminated[bas], tu = s.truncated[bs], wr = wr_p[bs];
    double cur = s.st.cur_return[bas];
    int32_t len = s.st.cur_length[bs];
    bool over = s.st.over[bs] != 0;
    int t = 0;
    do {                                                                  // (steps >= 1: the launcher returns before a launch otherwise)
        const int64_t tb = (int64_t)t * B + b, tba = (int64_t)t * BA + ba;
        // the next step's inputs (the last step: its own again), requested before this one is applied
        const int64_t tn = t + 1 < s.steps ? t + 1 : t;
        const double r_n = s.reward[tn * BA + bas];
        const uint32_t te_n = s.terminated[tn * BA + bas], tu_n = s.truncated[tn * B + bs], wr_n = wr_p[tn * B + bs];
        const uint64_t term_bits = __builtin_amdgcn_ballot_w64(live && te != 0);
        const bool all_term = ((term_bits >> sh) & ones) == ones;

        int32_t aborted = 0;
        if (mode == MGX_RESTART_BEFORE && wr) {                           // restarted before this step
            if (!over && len > 0) { aborted++; cur = 0.0; len = 0; }
            over = false;
        }
        bool closing = false;
        double ep_ret = 0.0;
        int32_t ep_len = 0;
        if (live && !over) {                                              // (an env that was over on entry: a step past the end)
            cur = cur + r;
            len++;
            closing = tu != 0 || all_term;
            ep_ret = cur; ep_len = len;
        }
        const uint64_t pos_bits = __builtin_amdgcn_ballot_w64(closing && ep_ret > 0.0);
        if (closing) {
            s.st.last_return[ba] = ep_ret;
            s.st.sum_return[ba] = s.st.sum_return[ba] + ep_ret;
            if (lead) {
                s.st.last_length[b] = ep_len;
                s.st.sum_length[b] += ep_len;
                int32_t *c = s.st.counts + b * 4;
                c[0] += 1;
                if (all_term) c[1] += 1;
                if ((pos_bits >> sh) & ones) c[2] += 1;
            }
            cur = 0.0; len = 0; over = true;
        }
        if (live) {
            if (s.tr.episode_return) s.tr.episode_return[tba] = closing ? ep_ret : 0.0;
            if (lead) {
                if (s.tr.closed) s.tr.closed[tb] = (uint8_t)closing;
                if (s.tr.episode_length) s.tr.episode_length[tb] = closing ? ep_len : 0;
            }
        }
        if (mode == MGX_RESTART_AFTER && wr) {                            // regenerated after this step
            if (!over && len > 0) { aborted++; cur = 0.0; len = 0; }
            over = false;
        }
        if (lead && aborted) s.st.counts[b * 4 + 3] += aborted;
        r = r_n; te = te_n; tu = tu_n; wr = wr_n;
    } while (++t < s.steps);
    if (live) {
        s.st.cur_return[ba] = cur;
        if (lead) {
            s.st.cur_length[b] = len;
            s.st.over[b] = (uint8_t)over;
        }
    }
}

struct RestartArgs {
    int64_t batch;
    int32_t A;
    const uint8_t *select;
    MgxEpisodeStats st;
};

__global__ __launch_bounds__(256) void episode_restart_kernel(const RestartArgs s) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool chosen = b < s.batch && (s.select == nullptr || s.select[b] != 0);
    if (__builtin_amdgcn_ballot_w64(chosen) == 0) return;
    if (!chosen) return;
    if (s.st.over[b] == 0 && s.st.cur_length[b] > 0) {                    // a running episode is discarded
        s.st.counts[b * 4 + 3] += 1;
        s.st.cur_length[b] = 0;
        for (int a = 0; a < s.A; ++a) s.st.cur_return[b * s.A + a] = 0.0;
    }
    s.st.over[b] = 0;
}

int check_stats(const MgxSpec *spec, int64_t batch, const MgxEpisodeStats *st) {
    if (!spec || batch < 0) return MGX_ERR_INVALID_ARGUMENT;
    if (spec->num_agents < 1 || spec->num_agents > MGX_MAX_AGENTS) return MGX_ERR_INVALID_ARGUMENT;
    if (batch == 0) return MGX_OK;
    if (!st || !st->cur_return || !st->cur_length || !st->over || !st->last_return || !st->last_length || !st->sum_return
        || !st->sum_length || !st->counts)
        return MGX_ERR_INVALID_ARGUMENT;
    if (misaligned(st->cur_return, 8) || misaligned(st->last_return, 8) || misaligned(st->sum_return, 8) || misaligned(st->sum_length, 8)
        || misaligned(st->cur_length, 4) || misaligned(st->last_length, 4) || misaligned(st->counts, 4))
        return MGX_ERR_INVALID_ARGUMENT;
    return MGX_OK;
}

}  // namespace

extern "C" {

int mgx_episode_stats(const MgxSpec *spec, int64_t batch, int32_t steps, const double *reward, const uint8_t *terminated,
                      const uint8_t *truncated, const uint8_t *was_reset, int32_t restart, const MgxEpisodeStats *stats,
                      const MgxEpisodeTrace *trace, void *stream) {
    if (!spec || batch < 0 || steps < 0) return MGX_ERR_INVALID_ARGUMENT;
    if (spec->num_agents < 1 || spec->num_agents > MGX_MAX_AGENTS) return MGX_ERR_INVALID_ARGUMENT;
    if (restart != MGX_RESTART_NONE && restart != MGX_RESTART_BEFORE && restart != MGX_RESTART_AFTER) return MGX_ERR_INVALID_ARGUMENT;
    if (batch == 0 || steps == 0) return MGX_OK;
    if (const int rc = check_stats(spec, batch, stats)) return rc;
    if (!reward || !terminated || !truncated || (restart != MGX_RESTART_NONE && !was_reset)) return MGX_ERR_INVALID_ARGUMENT;
    if (misaligned(reward, 8)) return MGX_ERR_INVALID_ARGUMENT;
    if (trace && (misaligned(trace->episode_return, 8) || misaligned(trace->episode_length, 4))) return MGX_ERR_INVALID_ARGUMENT;
    const int A = spec->num_agents, G = 64 / A;
    const int64_t waves = (batch + G - 1) / G;
    if (waves > INT_MAX) return MGX_ERR_UNSUPPORTED;
    const StatsArgs args{batch, A, G, steps, restart, reward, terminated, truncated, restart != MGX_RESTART_NONE ? was_reset : nullptr,
                         *stats, trace ? *trace : MgxEpisodeTrace{nullptr, nullptr, nullptr}};
    hipLaunchKernelGGL(episode_stats_kernel, dim3((unsigned)((waves + kStatsWaves - 1) / kStatsWaves)), dim3(64 * kStatsWaves), 0,
                       static_cast<hipStream_t>(stream), args);
    return finish_launch();
}

int mgx_episode_restart(const MgxSpec *spec, int64_t batch, const uint8_t *select, const MgxEpisodeStats *stats, void *stream) {
    if (const int rc = check_stats(spec, batch, stats)) return rc;
    if (batch == 0) return MGX_OK;
    if ((batch + 63) / 64 > INT_MAX) return MGX_ERR_UNSUPPORTED;
    const RestartArgs args{batch, spec->num_agents, select, *stats};
    hipLaunchKernelGGL(episode_restart_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       args);
    return finish_launch();
}

}  // extern "C"
