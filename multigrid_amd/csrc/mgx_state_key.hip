// mgx_state_key.hip -- 64-bit keys of env states and of agent views on the device (include/mgx.h: "STATE KEYS", mgx_state_key,
// mgx_obs_key), gfx950.  The rule itself -- the mixer, the words, the canonical cell of the three cell formats -- is mgx_state_key.h.
//
//   state_key_kernel<CB, VecT>   keys of n chosen rows of a state set (MgxEnvRows: a live batch or a snapshot).  A wavefront owns
//                           `run` consecutive envs (mgx_aux_geom.h: state_key_geom -- env_copy's runs of about 4 KiB of tile bytes)
//                           and every env a group of `group` lanes, a power of two: one lane per env at run = 64, the whole
//                           wavefront at run = 1.  Each lane of a group reads the env's index itself (one address per group: a
//                           broadcast) and range-checks it; a bad index is counted by the group's first lane and its key is left
//                           alone.  Lane k then takes the chunks k, k + group, ... of the env's cells -- a chunk is ONE load of the
//                           widest unit VecT that divides the tile size and the base address (state_key_unit), or, where that is
//                           narrower than a key word (two cells), the pieces of one word -- in rounds of kRound chunks, every load
//                           of a round issued before its mixing.  The kernel is bound by the VALU, not by the loads (two 64-bit
//                           multiplies a word: three quarter-rate instructions each), so the cells are made canonical a dword at
//                           a time: two 16-bit cells by five masked shifts (key_pair16), four compact cells by two v_perm_b32
//                           table look-ups (key_quad8).  Then the env's small words (agent rows, aux, step count, rng: one
//                           dword load each) the same way.  The lanes' partial keys meet in an XOR butterfly over the group
//                           (__shfl_xor: XOR makes the order free), and the group's first lane stores the 8 bytes.  No LDS, no
//                           inter-wavefront traffic but the two `bad` words (mgx_env_rows.h: count_bad).
//   obs_key_kernel          keys of n views u8[v,v,3] + their directions, the same way: a group of lanes (obs_key_group) per view,
//                           lane k takes the view's dwords k, k + group, ...  A view row is 3 * v * v bytes, so it is dword-aligned
//                           only every fourth view: the whole dwords are loaded at byte alignment (gfx950 serves a misaligned
//                           global dword load), the tail's bytes one by one -- no byte beyond the view is read.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mgx_aux_geom.h"
#include "mgx_host.h"
#include "mgx_state_key.h"

namespace {

using namespace mgx;

constexpr int kKeyWpb = kEnvCopyWpb;    // wavefronts per workgroup
constexpr int kRound = 4;               // chunks per lane in flight: loads of a round, then its mixing

struct StateKeyArgs {
    int64_t n;
    int32_t run, group, group_shift;    // envs per wavefront; lanes per env = 1 << group_shift
    int32_t A, HW, chunks, small;       // chunks of cells per env; small words per env
    uint32_t flags;
    int64_t tile_bytes;
    uint64_t salt;
    MgxEnvRows src;
    const int64_t *src_idx;
    int64_t *keys;
    int32_t *bad;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// what one lane holds of the cells at a time: kBytes of a tile, kWords key words
template <int CB, typename VecT>
struct KeyChunk {
    static constexpr int kVec = (int)sizeof(VecT);
    static constexpr int kBytes = CB == 3 ? 6 : (kVec > 2 * CB ? kVec : 2 * CB);
    static constexpr int kLoads = kBytes / kVec;
    static constexpr int kCells = kBytes / CB;
    static constexpr int kWords = kCells / 2;
    static constexpr int kRegs = (kBytes + 3) / 4;
    uint32_t w[kRegs];
};

template <int CB, typename VecT>
__device__ __forceinline__ void load_chunk(KeyChunk<CB, VecT> &r, const uint8_t *tile, int c, int tile_bytes) {
    using K = KeyChunk<CB, VecT>;
    if constexpr (K::kLoads == 1) {
        const VecT v = reinterpret_cast<const VecT *>(tile)[c];
        if constexpr (sizeof(VecT) >= 4) __builtin_memcpy(r.w, &v, sizeof(VecT));
        else r.w[0] = (uint32_t)v;
    } else {                                                      // a unit below a key word: its pieces, none beyond the tile
        uint64_t acc = 0;
#pragma unroll
        for (int l = 0; l < K::kLoads; ++l) {
            const int off = c * K::kBytes + l * K::kVec;
            const uint64_t v = off < tile_bytes ? (uint64_t)*reinterpret_cast<const VecT *>(tile + off) : 0ull;
            acc |= v << (8 * l * K::kVec);
        }
        r.w[0] = (uint32_t)acc;
        if constexpr (K::kRegs > 1) r.w[1] = (uint32_t)(acc >> 32);
    }
}

// the payload of word j of a chunk: its two cells, canonical -- a dword at a time for the 16-bit and the compact cells
template <int CB, typename VecT>
__device__ __forceinline__ uint32_t chunk_payload(const KeyChunk<CB, VecT> &r, int j) {
    if constexpr (CB == 2) {
        return key_pair16(r.w[j]);
    } else if constexpr (CB == 1) {
        uint32_t w0, w1;
        key_quad8(r.w[j >> 1], w0, w1);
        return (j & 1) ? w1 : w0;
    } else {                                                      // byte triples: one word a chunk, 6 bytes
        const uint32_t lo = r.w[0], hi = (r.w[0] >> 24) | (r.w[1] << 8);
        return key_cell24(lo, lo >> 8, lo >> 16) | (key_cell24(hi, hi >> 8, hi >> 16) << 16);
    }
}

template <int CB, typename VecT>
__device__ __forceinline__ uint64_t mix_chunk(const KeyChunk<CB, VecT> &r, int c, int HW, uint64_t salt) {
    using K = KeyChunk<CB, VecT>;
    uint64_t x = 0;
#pragma unroll
    for (int j = 0; j < K::kWords; ++j) {
        uint32_t payload = chunk_payload(r, j);
        if constexpr (K::kWords == 1)                             // (wider chunks divide an even number of cells; the pieces of
            if (2 * c + 1 >= HW) payload |= KEY_NO_CELL << 16;    //  a cell that is not there were loaded as zeros)
        x ^= key_term(KEY_TAG_CELLS, (uint32_t)(c * K::kWords + j), payload, salt);
    }
    return x;
}

// small word t of row s: the agent rows' dwords, the four of aux, the step count, the eight of rng
__device__ __forceinline__ uint32_t load_small(const StateKeyArgs &a, int64_t s, int t) {
    const int nag = 2 * a.A;
    if (t < nag) return reinterpret_cast<const uint32_t *>(a.src.agents)[s * nag + t];
    t -= nag;
    if (t < 4) return a.src.aux ? reinterpret_cast<const uint32_t *>(a.src.aux)[s * 4 + t] : 0u;
    t -= 4;
    if ((a.flags & MGX_KEY_STEP_COUNT) && t == 0) return (uint32_t)a.src.step_count[s];
    t -= (int)(a.flags & MGX_KEY_STEP_COUNT);
    return reinterpret_cast<const uint32_t *>(a.src.rng)[s * 8 + t];
}
__device__ __forceinline__ uint64_t mix_small(const StateKeyArgs &a, int t, uint32_t payload) {
    const int nag = 2 * a.A;
    if (t < nag) return key_term(KEY_TAG_AGENTS, (uint32_t)t, payload, a.salt);
    t -= nag;
    if (t < 4) return key_term(KEY_TAG_AUX, (uint32_t)t, payload, a.salt);
    t -= 4;
    if ((a.flags & MGX_KEY_STEP_COUNT) && t == 0) return key_term(KEY_TAG_STEP, 0u, payload, a.salt);
    t -= (int)(a.flags & MGX_KEY_STEP_COUNT);
    return key_term(KEY_TAG_RNG, (uint32_t)t, payload, a.salt);
}

// XOR over the lanes of a group (a power of two, aligned): every lane of the wavefront takes part
__device__ __forceinline__ uint64_t group_xor(uint64_t x, int group) {
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    for (int off = group >> 1; off > 0; off >>= 1) {
        lo ^= (uint32_t)__shfl_xor((int)lo, off);
        hi ^= (uint32_t)__shfl_xor((int)hi, off);
    }
    return lo | ((uint64_t)hi << 32);
}

template <int CB, typename VecT>
__global__ __launch_bounds__(64 * kKeyWpb) void state_key_kernel(const StateKeyArgs a) {
    using K = KeyChunk<CB, VecT>;
    const RowWave w = row_wave<kKeyWpb>(a.run);
    if (w.p0 >= a.n) return;                                      // (the lanes below stay together up to the butterfly)
    const int e = w.lane >> a.group_shift, k = w.lane & (a.group - 1);
    const int64_t i = w.p0 + e;
    int64_t s = 0;
    bool ok = false;
    if (e < a.run && i < a.n) ok = pick_row(a.src_idx, i, a.src.rows, k == 0, a.bad, s);   // (a bad index: its key is left alone)
    uint64_t key = 0;
    if (ok) {
        const uint8_t *tile = reinterpret_cast<const uint8_t *>(a.src.cells) + s * a.tile_bytes;
        const int step = a.group * kRound;
        for (int c0 = k; c0 < a.chunks; c0 += step) {
            K r[kRound];
#pragma unroll
            for (int j = 0; j < kRound; ++j)
                if (c0 + j * a.group < a.chunks) load_chunk<CB, VecT>(r[j], tile, c0 + j * a.group, (int)a.tile_bytes);
#pragma unroll
            for (int j = 0; j < kRound; ++j)
                if (c0 + j * a.group < a.chunks) key ^= mix_chunk<CB, VecT>(r[j], c0 + j * a.group, a.HW, a.salt);
        }
        for (int t0 = k; t0 < a.small; t0 += step) {
            uint32_t w[kRound];
#pragma unroll
            for (int j = 0; j < kRound; ++j)
                if (t0 + j * a.group < a.small) w[j] = load_small(a, s, t0 + j * a.group);
#pragma unroll
            for (int j = 0; j < kRound; ++j)
                if (t0 + j * a.group < a.small) key ^= mix_small(a, t0 + j * a.group, w[j]);
        }
    }
    key = group_xor(key, a.group);
    if (ok && k == 0) a.keys[i] = (int64_t)key;
}

struct ObsKeyArgs {
    int64_t n;
    int32_t group, group_shift, bytes, words;     // lanes per view; bytes and dwords (the tail's included) of a view
    uint64_t salt;
    const uint8_t *obs, *dir;
    int64_t *keys;
};

// BYTES: every byte by a load of its own (the tools' build measures it against the dwords: tools/state_key_bench.py)
template <bool BYTES>
__device__ __forceinline__ uint32_t load_view_word(const uint8_t *img, int j, int bytes) {
    uint32_t w = 0;
    if (!BYTES && 4 * j + 4 <= bytes) {
        __builtin_memcpy(&w, img + 4 * j, 4);                     // (byte-aligned: one global dword load on gfx950)
    } else {
        for (int b = 0; b < 4 && 4 * j + b < bytes; ++b) w |= (uint32_t)img[4 * j + b] << (8 * b);
    }
    return w;
}

template <bool BYTES>
__global__ __launch_bounds__(64 * kKeyWpb) void obs_key_kernel(const ObsKeyArgs a) {
    const RowWave w = row_wave<kKeyWpb>(64 >> a.group_shift);
    if (w.p0 >= a.n) return;
    const int k = w.lane & (a.group - 1);
    const int64_t i = w.p0 + (w.lane >> a.group_shift);
    const bool ok = i < a.n;
    uint64_t key = 0;
    if (ok) {
        const uint8_t *img = a.obs + i * a.bytes;
        const int step = a.group * kRound;
        for (int j0 = k; j0 < a.words; j0 += step) {
            uint32_t w[kRound];
#pragma unroll
            for (int j = 0; j < kRound; ++j)
                if (j0 + j * a.group < a.words) w[j] = load_view_word<BYTES>(img, j0 + j * a.group, a.bytes);
#pragma unroll
            for (int j = 0; j < kRound; ++j)
                if (j0 + j * a.group < a.words) key ^= key_term(KEY_TAG_IMAGE, (uint32_t)(j0 + j * a.group), w[j], a.salt);
        }
        if (k == 0) key ^= key_term(KEY_TAG_DIR, 0u, a.dir[i], a.salt);
    }
    key = group_xor(key, a.group);
    if (ok && k == 0) a.keys[i] = (int64_t)key;
}

typedef void (*StateKeyKernel)(const StateKeyArgs);

// the kernel's instantiation for a cell format and a load unit of 16 / 8 / 4 / 2 / 1 bytes (mgx_aux_geom.h: state_key_unit)
StateKeyKernel state_key_by_unit(int cb, int unit) {
    if (cb == 3) return unit == 2 ? state_key_kernel<3, uint16_t> : state_key_kernel<3, uint8_t>;
    if (cb == 1)
        return unit == 16 ? state_key_kernel<1, u32x4> : unit == 8 ? state_key_kernel<1, uint64_t> : unit == 4 ? state_key_kernel<1, uint32_t>
               : unit == 2 ? state_key_kernel<1, uint16_t> : state_key_kernel<1, uint8_t>;
    return unit == 16 ? state_key_kernel<2, u32x4> : unit == 8 ? state_key_kernel<2, uint64_t> : unit == 4 ? state_key_kernel<2, uint32_t>
                                                                                                           : state_key_kernel<2, uint16_t>;
}

#if defined(MGX_DEBUG_KNOBS) && MGX_DEBUG_KNOBS
int g_obs_key_bytes = 0;                // the tools' build: mgx_obs_key loads the views byte by byte

// a read-only stream for the tools' build: 16-byte loads, grid-stride, XORed; one store a wavefront so that nothing is elided
__global__ __launch_bounds__(256) void stream_read_kernel(const u32x4 *p, int64_t n16, uint32_t *out) {
    u32x4 acc = {0, 0, 0, 0};
    const int64_t stride = (int64_t)gridDim.x * 256 * 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 * 4 + threadIdx.x; i < n16; i += stride) {
        u32x4 r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + 256 * k < n16) r[k] = p[i + 256 * k];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + 256 * k < n16) acc ^= r[k];
    }
    const uint32_t x = (uint32_t)group_xor(acc.x ^ acc.y ^ acc.z ^ acc.w, 64);
    if ((threadIdx.x & 63) == 0) out[(blockIdx.x * 256 + threadIdx.x) >> 6] = x;
}
#endif

}  // namespace

extern "C" {

#if defined(MGX_DEBUG_KNOBS) && MGX_DEBUG_KNOBS
void mgx_debug_obs_key_bytes(int on) { g_obs_key_bytes = on; }
// reads `bytes` (a multiple of 16, 16-byte aligned) once; out: u32[4 * blocks], blocks = mgx_debug_stream_read_blocks()
int mgx_debug_stream_read_blocks(void) { return 256 * 16; }
int mgx_debug_stream_read(const void *p, int64_t bytes, uint32_t *out, void *stream) {
    hipLaunchKernelGGL(stream_read_kernel, dim3(256 * 16), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const u32x4 *>(p), bytes / 16, out);
    return finish_launch();
}
#endif

int mgx_state_key(const MgxSpec *spec, int64_t n, const MgxEnvRows *src, const int64_t *src_idx, uint32_t flags, uint64_t salt,
                  int64_t *keys, int32_t *bad, void *stream) {
    if (check_rows_spec(spec) || n < 0 || !src) return MGX_ERR_INVALID_ARGUMENT;
    if (src->rows < 0 || (flags & ~(uint32_t)(MGX_KEY_STEP_COUNT | MGX_KEY_RNG))) return MGX_ERR_INVALID_ARGUMENT;
    if (n == 0) return MGX_OK;
    const int cb = cell_bytes(spec->cell_bytes);
    const uint32_t read = ROWS_CELLS | ROWS_AGENTS | ROWS_RNG | ROWS_STEP_COUNT;
    if (check_rows(*src, read, read | ROWS_AUX, cb) || !keys || misaligned(keys, 8)) return MGX_ERR_INVALID_ARGUMENT;
    if (const int rc = check_rows_n(n, src_idx, bad, kKeyWpb)) return rc;
    const int64_t cells = (int64_t)spec->width * spec->height;
    if (cells > 2 * 65536) return MGX_ERR_UNSUPPORTED;            // (a cell word's index is 16 bits wide)
    const int HW = (int)cells, tile_bytes = HW * cb;
    const StateKeyGeom g = state_key_geom(tile_bytes, n);
    if (g.blocks > INT_MAX) return MGX_ERR_UNSUPPORTED;
    const int unit = state_key_unit(cb, tile_bytes, reinterpret_cast<uintptr_t>(src->cells));
    const int chunk = state_key_chunk_bytes(cb, unit);
    const int small = 2 * spec->num_agents + 4 + ((flags & MGX_KEY_STEP_COUNT) ? 1 : 0) + ((flags & MGX_KEY_RNG) ? 8 : 0);
    const StateKeyArgs args{n, g.run, g.group, log2_of(g.group), spec->num_agents, HW, (tile_bytes + chunk - 1) / chunk, small, flags,
                            tile_bytes, salt, *src, src_idx, keys, bad};
    hipLaunchKernelGGL(state_key_by_unit(cb, unit), dim3((unsigned)g.blocks), dim3(64 * kKeyWpb), 0, static_cast<hipStream_t>(stream),
                       args);
    return finish_launch();
}

int mgx_obs_key(const MgxSpec *spec, int64_t n_views, const uint8_t *obs, const uint8_t *dir, uint64_t salt, int64_t *keys,
                void *stream) {
    if (!spec || n_views < 0) return MGX_ERR_INVALID_ARGUMENT;
    if (spec->view_size < 1 || spec->view_size > MGX_MAX_VIEW) return MGX_ERR_INVALID_ARGUMENT;
    if (n_views == 0) return MGX_OK;
    if (!obs || !dir || !keys || misaligned(keys, 8)) return MGX_ERR_INVALID_ARGUMENT;
    const int bytes = 3 * spec->view_size * spec->view_size;
    const int group = obs_key_group(bytes), per = 64 / group;
    const int64_t nwaves = (n_views + per - 1) / per, blocks = (nwaves + kKeyWpb - 1) / kKeyWpb;
    if (blocks > INT_MAX) return MGX_ERR_UNSUPPORTED;
    const ObsKeyArgs args{n_views, group, log2_of(group), bytes, (bytes + 3) / 4, salt, obs, dir, keys};
#if defined(MGX_DEBUG_KNOBS) && MGX_DEBUG_KNOBS
    if (g_obs_key_bytes) {
        hipLaunchKernelGGL(obs_key_kernel<true>, dim3((unsigned)blocks), dim3(64 * kKeyWpb), 0, static_cast<hipStream_t>(stream), args);
        return finish_launch();
    }
#endif
    hipLaunchKernelGGL(obs_key_kernel<false>, dim3((unsigned)blocks), dim3(64 * kKeyWpb), 0, static_cast<hipStream_t>(stream), args);
    return finish_launch();
}

}  // extern "C"
