// mgx_select.hip -- the device selection (include/mgx.h: "SELECTION", mgx_select), gfx950: the k best of n by (score, index), as an
// order-preserving compaction of fixed length with the count kept on the device.  The rule -- the biased key, its digits, the
// threshold T and the quota r, chosen-or-not and the place of a chosen item -- is mgx_select.h; this file is its parallel form.
//
// A workgroup of 256 threads takes a CHUNK of whole tiles of 256 consecutive items, one item per thread and round; at most 1024
// chunks, so every sum over chunks is one short read per workgroup.  The launches of a call, all on the caller's stream:
//
//   select_zero_kernel        the three histograms of the work buffer := 0                                         (scored calls only)
//   select_hist_kernel<0>     the histogram of the top digit over the candidates: per workgroup in LDS, then one global add per
//                             non-empty bin                                                                        (scored calls only)
//   select_hist_kernel<1|2>   every workgroup re-derives, from the bins of the pass before, the digit that holds the rank (a scan
//                             of the bins: 8 per thread), and counts the next digit of the candidates that match the digits so
//                             far; workgroup 0 leaves prefix and rank in the state words for the launch after          (scored only)
//   select_count_kernel       derives the last digit, hence T and r, the same way; per chunk lt = #{u < T}, eq = #{u == T}
//   select_scatter_kernel     the exclusive sums of lt and eq over the chunks before its own, then per tile ballot + popcount:
//                             item i is chosen iff u < T or (u == T and eq_before < r), its place is lt_before + min(eq_before, r);
//                             the pads index[m..k) = fill are spread over the grid, one thread writes count
//   select_fill_kernel        n == 0: index := fill, count := {0, 0}
//
// Six launches with scores, two without (the select passes vanish: every key is 0, T = 0, r = m) -- a function of the arguments, never
// of the data.  THE ONLY HAND-OFF BETWEEN WORKGROUPS IS A KERNEL BOUNDARY: no flag, no fence, no look-back, no spin, and no launch reads
// a word of the work buffer that it also writes.  The state words (work[0..16)):
//   [0] |C|  [1] m  [2] prefix after pass 0  [3] rank after pass 0     written by select_hist_kernel<1>, workgroup 0
//   [4] prefix after pass 1  [5] rank after pass 1                     written by select_hist_kernel<2>, workgroup 0
//   [6] T  [7] r                                                       written by select_count_kernel, workgroup 0
// then the histograms (2048 + 2048 + 1024 words) and lt[chunks], eq[chunks].  Everything the call reads it has written itself first:
// the work buffer's contents on entry are arbitrary, and a captured call replays on new data.
//
// The histograms take integer adds, so their sums do not depend on the order of arrival, and every output position is computed, not
// claimed: the outputs are a pure function of the inputs.  A wavefront whose candidates all fall into one bin (every score equal, a
// level's narrow spread in the upper passes) adds once, not 64 times to one LDS word.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mgx_host.h"
#include "mgx_select.h"

namespace {

using namespace mgx;

constexpr int kThreads = SELECT_TILE;          // one item per thread and round
constexpr int kWaves = kThreads / 64;
constexpr int kFillBlocks = 1024;              // the pads of the n == 0 form: grid-stride over k

enum { ST_CANDS = 0, ST_M = 1, ST_PREFIX0 = 2, ST_RANK0 = 3, ST_PREFIX1 = 4, ST_RANK1 = 5, ST_T = 6, ST_R = 7 };

struct SelectArgs {
    int64_t n, k, fill;
    const int32_t *score;
    const uint8_t *keep;
    const int64_t *values;
    int64_t *index;
    int32_t *count;
    uint32_t *state, *hist, *chunk_lt, *chunk_eq;
    int64_t tiles_per_chunk;
    int32_t chunks;
};

// the sum of v over the threads before this one, and over all threads; `lds` holds kWaves words nobody else uses meanwhile
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *lds, uint32_t *total) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t c = lds[w];
        if (w < wave) base += c;
        all += c;
    }
    *total = all;
    return base + incl - v;
}

struct Found { uint32_t prefix, rank; };

// What the launch after pass STAGE - 1 knows: the digit of that pass that holds the rank, joined to the digits before it, and the rank
// inside that digit's bin.  Every workgroup computes the same; `lds` holds kWaves + 2 words.
template <int STAGE> __device__ __forceinline__ Found select_derive(const SelectArgs &a, uint32_t *lds) {
    constexpr int pass = STAGE - 1, bins = pass == 2 ? 1024 : 2048, per = bins / kThreads;
    const uint32_t *hist = a.hist + select_hist_offset(pass) + (int)threadIdx.x * per;
    uint32_t mine = 0;
#pragma unroll
    for (int b = 0; b < per; ++b) mine += hist[b];
    uint32_t total;
    const uint32_t base = block_exclusive(mine, lds, &total);
    Found f;
    const uint32_t prefix = STAGE == 1 ? 0u : a.state[STAGE == 2 ? ST_PREFIX0 : ST_PREFIX1];
    const uint32_t rank = STAGE == 1 ? (uint32_t)((int64_t)total < a.k ? (int64_t)total : a.k) : a.state[STAGE == 2 ? ST_RANK0 : ST_RANK1];
    uint32_t bin, before;
    if (select_find_bin(hist, (int)threadIdx.x * per, per, base, rank, &bin, &before)) {       // (exactly one thread)
        lds[kWaves] = bin;
        lds[kWaves + 1] = before;
    }
    __syncthreads();
    f.prefix = select_extend(prefix, pass, lds[kWaves]);
    f.rank = rank - lds[kWaves + 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (STAGE == 1) {
            a.state[ST_CANDS] = total;
            a.state[ST_M] = rank;
        }
        a.state[STAGE == 1 ? ST_PREFIX0 : (STAGE == 2 ? ST_PREFIX1 : ST_T)] = f.prefix;
        a.state[STAGE == 1 ? ST_RANK0 : (STAGE == 2 ? ST_RANK1 : ST_R)] = f.rank;
    }
    return f;
}

__global__ __launch_bounds__(kThreads) void select_zero_kernel(const SelectArgs a) {
    const int w = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (w < SELECT_HIST_WORDS) a.hist[w] = 0;
}

template <int PASS> __global__ __launch_bounds__(kThreads) void select_hist_kernel(const SelectArgs a) {
    constexpr int bins = PASS == 2 ? 1024 : 2048;
    __shared__ uint32_t local[bins];
    __shared__ uint32_t sc[kWaves + 2];
    for (int b = (int)threadIdx.x; b < bins; b += kThreads) local[b] = 0;
    uint32_t prefix = 0;
    if constexpr (PASS > 0) prefix = select_derive<PASS>(a, sc).prefix;
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63);
    const int64_t first = (int64_t)blockIdx.x * a.tiles_per_chunk * kThreads;
    for (int64_t t = 0; t < a.tiles_per_chunk; ++t) {
        const int64_t tile = first + t * kThreads;
        if (tile >= a.n) break;
        const int64_t i = tile + threadIdx.x;
        bool match = i < a.n && (!a.keep || a.keep[i] != 0);
        uint32_t d = 0;
        if (match) {
            const uint32_t u = select_key(a.score[i]);
            match = select_prefix(u, PASS) == prefix;
            d = select_digit(u, PASS);
        }
        const unsigned long long in = __ballot(match);
        if (in == 0) continue;
        const int lead = __ffsll(in) - 1;
        const uint32_t d0 = (uint32_t)__shfl((int)d, lead);
        if (__ballot(match && d == d0) == in) {                    // one bin for the whole wavefront: one add
            if (lane == lead) atomicAdd(&local[d0], (uint32_t)__popcll(in));
        } else if (match) {
            atomicAdd(&local[d], 1u);
        }
    }
    __syncthreads();
    uint32_t *hist = a.hist + select_hist_offset(PASS);
    for (int b = (int)threadIdx.x; b < bins; b += kThreads) {
        const uint32_t c = local[b];
        if (c) atomicAdd(hist + b, c);
    }
}

template <bool SCORED> __global__ __launch_bounds__(kThreads) void select_count_kernel(const SelectArgs a) {
    __shared__ uint32_t sums[kWaves][2];
    uint32_t T = 0;
    if constexpr (SCORED) {
        __shared__ uint32_t sc[kWaves + 2];
        T = select_derive<3>(a, sc).prefix;
    }
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t first = (int64_t)blockIdx.x * a.tiles_per_chunk * kThreads;
    uint32_t lt = 0, eq = 0;                                       // of this wavefront (uniform)
    for (int64_t t = 0; t < a.tiles_per_chunk; ++t) {
        const int64_t tile = first + t * kThreads;
        if (tile >= a.n) break;
        const int64_t i = tile + threadIdx.x;
        const bool cand = i < a.n && (!a.keep || a.keep[i] != 0);
        const uint32_t u = SCORED && cand ? select_key(a.score[i]) : 0u;
        lt += (uint32_t)__popcll(__ballot(cand && u < T));
        eq += (uint32_t)__popcll(__ballot(cand && u == T));
    }
    if (lane == 0) {
        sums[wave][0] = lt;
        sums[wave][1] = eq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t l = 0, e = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            l += sums[w][0];
            e += sums[w][1];
        }
        a.chunk_lt[blockIdx.x] = l;
        a.chunk_eq[blockIdx.x] = e;
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

template <bool SCORED> __global__ __launch_bounds__(kThreads) void select_scatter_kernel(const SelectArgs a) {
    __shared__ uint32_t sums[kWaves][3];
    __shared__ uint32_t tile_sums[2][kWaves][2];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    // lt and eq of the chunks before this one; eq of all chunks (an unscored call's |C|)
    uint32_t run_lt = 0, run_eq = 0, all_eq = 0;
    for (int j = (int)threadIdx.x; j < a.chunks; j += kThreads) {
        const uint32_t l = a.chunk_lt[j], e = a.chunk_eq[j];
        if (j < (int)blockIdx.x) {
            run_lt += l;
            run_eq += e;
        }
        all_eq += e;
    }
    run_lt = wave_sum(run_lt);
    run_eq = wave_sum(run_eq);
    all_eq = wave_sum(all_eq);
    if (lane == 0) {
        sums[wave][0] = run_lt;
        sums[wave][1] = run_eq;
        sums[wave][2] = all_eq;
    }
    __syncthreads();
    run_lt = run_eq = all_eq = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        run_lt += sums[w][0];
        run_eq += sums[w][1];
        all_eq += sums[w][2];
    }
    const uint32_t cands = SCORED ? a.state[ST_CANDS] : all_eq;
    const uint32_t m = SCORED ? a.state[ST_M] : (uint32_t)((int64_t)cands < a.k ? (int64_t)cands : a.k);
    const uint32_t T = SCORED ? a.state[ST_T] : 0u, r = SCORED ? a.state[ST_R] : m;

    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t first = (int64_t)blockIdx.x * a.tiles_per_chunk * kThreads;
    for (int64_t t = 0; t < a.tiles_per_chunk; ++t) {
        const int64_t tile = first + t * kThreads;
        if (tile >= a.n) break;
        const int64_t i = tile + threadIdx.x;
        const bool cand = i < a.n && (!a.keep || a.keep[i] != 0);
        const uint32_t u = SCORED && cand ? select_key(a.score[i]) : 0u;
        const unsigned long long lt_in = __ballot(cand && u < T), eq_in = __ballot(cand && u == T);
        uint32_t (*ts)[2] = tile_sums[t & 1];                       // (two buffers: a wavefront may be a round ahead, never two)
        if (lane == 0) {
            ts[wave][0] = (uint32_t)__popcll(lt_in);
            ts[wave][1] = (uint32_t)__popcll(eq_in);
        }
        __syncthreads();
        uint32_t lt_before = run_lt + (uint32_t)__popcll(lt_in & below), eq_before = run_eq + (uint32_t)__popcll(eq_in & below);
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t l = ts[w][0], e = ts[w][1];
            if (w < wave) {
                lt_before += l;
                eq_before += e;
            }
            run_lt += l;
            run_eq += e;
        }
        if (cand && select_chosen(u, T, r, eq_before)) {
            const int64_t at = (int64_t)select_place(lt_before, eq_before, r);
            if (at < a.k) a.index[at] = a.values ? a.values[i] : i;  // (at < m <= k by the rule)
        }
    }
    for (int64_t j = (int64_t)m + (int64_t)blockIdx.x * kThreads + threadIdx.x; j < a.k; j += (int64_t)gridDim.x * kThreads) a.index[j] = a.fill;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.count[0] = (int32_t)m;
        a.count[1] = (int32_t)cands;
    }
}

__global__ __launch_bounds__(kThreads) void select_fill_kernel(const SelectArgs a) {
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < a.k; j += (int64_t)gridDim.x * kThreads) a.index[j] = a.fill;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.count[0] = a.count[1] = 0;
}

template <typename K> int launch(K kernel, int64_t blocks, const SelectArgs &args, void *stream) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), args);
    return finish_launch();
}

}  // namespace

extern "C" {

size_t mgx_select_work_bytes(int64_t n) { return select_work_bytes(n); }

int mgx_select(int64_t n, const int32_t *score, const uint8_t *keep, const int64_t *values, int64_t k, int64_t fill, int64_t *index,
               int32_t *count, void *work, size_t work_bytes, void *stream) {
    if (n < 0 || k < 1 || (!score && !keep) || !index || !count) return MGX_ERR_INVALID_ARGUMENT;
    SelectArgs args{n, k, fill, score, keep, values, index, count, nullptr, nullptr, nullptr, nullptr, 0, 0};
    if (n == 0) {
        const int64_t tiles = select_tiles(k);
        return launch(select_fill_kernel, tiles < kFillBlocks ? tiles : kFillBlocks, args, stream);
    }
    if (!work || work_bytes < select_work_bytes(n) || misaligned(score, 4) || misaligned(values, 8) || misaligned(index, 8)
        || misaligned(count, 4) || misaligned(work, 16))
        return MGX_ERR_INVALID_ARGUMENT;
    if (n > (int64_t)INT_MAX || k > (int64_t)INT_MAX) return MGX_ERR_UNSUPPORTED;
    const int64_t chunks = select_chunks(n);
    args.state = static_cast<uint32_t *>(work);
    args.hist = args.state + SELECT_STATE_WORDS;
    args.chunk_lt = args.hist + SELECT_HIST_WORDS;
    args.chunk_eq = args.chunk_lt + chunks;
    args.tiles_per_chunk = select_tiles_per_chunk(n);
    args.chunks = (int32_t)chunks;
    int rc;
    if (score) {
        if ((rc = launch(select_zero_kernel, (SELECT_HIST_WORDS + kThreads - 1) / kThreads, args, stream)) != MGX_OK) return rc;
        if ((rc = launch(select_hist_kernel<0>, chunks, args, stream)) != MGX_OK) return rc;
        if ((rc = launch(select_hist_kernel<1>, chunks, args, stream)) != MGX_OK) return rc;
        if ((rc = launch(select_hist_kernel<2>, chunks, args, stream)) != MGX_OK) return rc;
        if ((rc = launch(select_count_kernel<true>, chunks, args, stream)) != MGX_OK) return rc;
        return launch(select_scatter_kernel<true>, chunks, args, stream);
    }
    if ((rc = launch(select_count_kernel<false>, chunks, args, stream)) != MGX_OK) return rc;
    return launch(select_scatter_kernel<false>, chunks, args, stream);
}

}  // extern "C"
