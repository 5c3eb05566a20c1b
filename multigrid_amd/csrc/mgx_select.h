// mgx_select.h -- the rule of the device selection (include/mgx.h: "SELECTION", mgx_select), stated once for both compilers: the kernels
// of mgx_select.hip bias, split, threshold and place with these functions, and g++ builds the same header into the stand-alone program
// of tests/test_select.py, which holds `select_serial` -- the serial statement over host arrays, by the same radix passes -- to a
// NumPy model of THE RULE (lexsort over the candidates, cut at k, sort the indices, pad).
//
// THE RULE.  Candidates C = { i < n : keep == NULL or keep[i] != 0 }, m = min(k, |C|).  Chosen are the m candidates smallest by the
// pair (score[i], i); index[0..m) holds them in ASCENDING i (values[i] in place of i when `values` is given), index[m..k) = fill,
// count = { m, |C| }.
//
// HOW.  With u the biased key of a score (unsigned order = signed order of the scores), let T be the m-th smallest u among the
// candidates and r = m - #{ candidates with u < T }: the QUOTA of the tie group at the threshold, 1 <= r <= #{ u == T } (m == 0: T = 0,
// r = 0).  Candidate i is chosen iff u < T, or u == T and fewer than r candidates before i have u == T; its place in `index` is
// #{ chosen before i } = lt_before(i) + min(eq_before(i), r).  T is found digit by digit, from the top: the histogram of the current
// digit over the candidates that match the digits found so far names the bin that holds the rank, and the rank inside that bin.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mgx.h"

#ifndef MGX_HD
#if defined(__HIPCC__)
#define MGX_HD __host__ __device__ __forceinline__
#else
#define MGX_HD inline
#endif
#endif

namespace mgx {

// ---- the key and its digits: three passes of 11, 11 and 10 bits, from the top -------------------------------------------------------
constexpr int SELECT_PASSES = 3;
constexpr int SELECT_MAX_BINS = 2048;
MGX_HD uint32_t select_key(int32_t score) { return (uint32_t)score ^ 0x80000000u; }
MGX_HD int select_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
MGX_HD int select_bins(int pass) { return pass == 2 ? 1024 : 2048; }
MGX_HD uint32_t select_digit(uint32_t u, int pass) { return (u >> select_shift(pass)) & (uint32_t)(select_bins(pass) - 1); }
// the digits above `pass`: what a key must share with the threshold's to be counted in that pass (pass 0: nothing, 0)
MGX_HD uint32_t select_prefix(uint32_t u, int pass) { return pass == 0 ? 0u : u >> select_shift(pass - 1); }
// the prefix after `pass` found the digit `bin`
MGX_HD uint32_t select_extend(uint32_t prefix, int pass, uint32_t bin) {
    return pass == 0 ? bin : (prefix << (select_shift(pass - 1) - select_shift(pass))) | bin;
}
// where the histogram of `pass` starts in the work buffer's histogram words
MGX_HD int select_hist_offset(int pass) { return pass * SELECT_MAX_BINS; }
constexpr int SELECT_HIST_WORDS = 2 * SELECT_MAX_BINS + 1024;

// ---- the threshold and the quota ----------------------------------------------------------------------------------------------------
// `rank` is 1-based inside the group the histogram counts (0: nothing is wanted).  The bin that holds it is the first whose inclusive
// sum reaches it; `before` is that bin's exclusive sum, and rank - before the rank inside the bin.  A thread of the kernels that owns
// the bins [first, first + count) with `base` items before them calls this on its own bins; the host calls it on all of them.
MGX_HD bool select_find_bin(const uint32_t *hist, int first, int count, uint32_t base, uint32_t rank, uint32_t *bin, uint32_t *before) {
    if (rank == 0) {
        if (first != 0) return false;
        *bin = 0;
        *before = 0;
        return true;
    }
    uint32_t sum = base;
    for (int b = 0; b < count; ++b) {
        const uint32_t c = hist[b];
        if (rank > sum && rank <= sum + c) {
            *bin = (uint32_t)(first + b);
            *before = sum;
            return true;
        }
        sum += c;
    }
    return false;
}

// is the candidate with key u, with eq_before candidates of key T before it, chosen?
MGX_HD bool select_chosen(uint32_t u, uint32_t T, uint32_t r, uint32_t eq_before) { return u < T || (u == T && eq_before < r); }
// ... and its place: the chosen before it
MGX_HD uint32_t select_place(uint32_t lt_before, uint32_t eq_before, uint32_t r) { return lt_before + (eq_before < r ? eq_before : r); }

// ---- the geometry of the launches and the work buffer --------------------------------------------------------------------------------
// A workgroup takes a CHUNK of whole tiles of SELECT_TILE consecutive items, one item per thread and round; there are at most
// SELECT_MAX_CHUNKS chunks, so that the sums over chunks stay one short read per workgroup however large n is.
constexpr int SELECT_TILE = 256;
constexpr int SELECT_MAX_CHUNKS = 1024;
constexpr int SELECT_STATE_WORDS = 16;         // work[0..16): what one launch leaves for the next (mgx_select.hip names the words)
MGX_HD int64_t select_tiles(int64_t n) { return (n + SELECT_TILE - 1) / SELECT_TILE; }
MGX_HD int64_t select_tiles_per_chunk(int64_t n) { return (select_tiles(n) + SELECT_MAX_CHUNKS - 1) / SELECT_MAX_CHUNKS; }
MGX_HD int64_t select_chunks(int64_t n) {
    const int64_t per = select_tiles_per_chunk(n);
    return per ? (select_tiles(n) + per - 1) / per : 0;
}
// words of 4 bytes: the state, the three histograms, lt and eq of every chunk; rounded up to 16 bytes.  Sized by min(tiles,
// SELECT_MAX_CHUNKS), which bounds the chunks and, unlike their number, never falls as n grows.
MGX_HD size_t select_work_bytes(int64_t n) {
    if (n < 0) n = 0;
    const int64_t most = select_tiles(n) < SELECT_MAX_CHUNKS ? select_tiles(n) : SELECT_MAX_CHUNKS;
    const size_t words = (size_t)SELECT_STATE_WORDS + (size_t)SELECT_HIST_WORDS + 2 * (size_t)most;
    return (words * 4 + 15) / 16 * 16;
}

// ---- the serial statement ------------------------------------------------------------------------------------------------------------
// score, keep, values nullable (not score and keep both); index i64[k], count i32[2].  `hist` is SELECT_MAX_BINS words of the caller's.
inline void select_serial(int64_t n, const int32_t *score, const uint8_t *keep, const int64_t *values, int64_t k, int64_t fill,
                          int64_t *index, int32_t *count, uint32_t *hist) {
    int64_t cands = 0;
    for (int64_t i = 0; i < n; ++i) cands += !keep || keep[i];
    const int64_t m = k < cands ? k : cands;
    uint32_t T = 0, r = (uint32_t)m;
    if (score) {
        uint32_t prefix = 0;
        for (int pass = 0; pass < SELECT_PASSES; ++pass) {
            const int bins = select_bins(pass);
            for (int b = 0; b < bins; ++b) hist[b] = 0;
            for (int64_t i = 0; i < n; ++i) {
                if (keep && !keep[i]) continue;
                const uint32_t u = select_key(score[i]);
                if (select_prefix(u, pass) == prefix) hist[select_digit(u, pass)] += 1;
            }
            uint32_t bin = 0, before = 0;
            select_find_bin(hist, 0, bins, 0, r, &bin, &before);
            prefix = select_extend(prefix, pass, bin);
            r -= before;
        }
        T = prefix;
    }
    uint32_t lt = 0, eq = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (keep && !keep[i]) continue;
        const uint32_t u = score ? select_key(score[i]) : 0u;
        if (select_chosen(u, T, r, eq)) index[select_place(lt, eq, r)] = values ? values[i] : i;
        lt += u < T;
        eq += u == T;
    }
    for (int64_t j = m; j < k; ++j) index[j] = fill;
    count[0] = (int32_t)m;
    count[1] = (int32_t)cands;
}

}  // namespace mgx
