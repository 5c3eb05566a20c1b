// mgx_key_table.hip -- the device key tables (include/mgx.h: "KEY TABLES", mgx_key_insert, mgx_key_lookup), gfx950.  The rule --
// the canonical key, home, the window, the tag word -- is mgx_key_table.h; this file is its concurrent form.  One thread per index,
// straight per-lane code: no LDS, no scratch, vector memory instructions and HIP atomics only.
//
//   key_place_kernel    the first launch of an insert.  A thread walks its key's window; per slot a PLAIN load first, then, only where
//                       that showed "empty", old = atomicCAS(&keys[s], 0, k), which both claims and reads at device scope.  The plain
//                       load is a saving in one direction only: another XCD's L2 (or this CU's L1) can show a stale "empty", and the
//                       CAS then tells the truth; it can never show a stale OTHER key or a stale absence of OUR key that matters,
//                       because a slot is written once -- any non-zero value ever read from a slot is the slot's value for good.
//                       The claiming thread stores born[s] = epoch; every walking thread does atomicMax(&tag[s], epoch << 32 | ~i)
//                       -- a later call beats an earlier one, within a call the smallest index wins -- and, unless
//                       MGX_KEY_NO_COUNT, atomicAdd(&visits[s], the indices it walks for); then every thread stores entry[i].
//   key_report_kernel   the second launch, after the kernel boundary has made the first one's stores and atomics visible on every
//                       XCD: is_new, first and visits of index i are read back from born, tag and visits of slot entry[i].
//   key_lookup_kernel   one launch, plain loads only, stops at the first empty slot (the invariant).
//
// NO THREAD EVER WAITS FOR ANOTHER THREAD'S STORE: there is no spin loop, no lock and no "slot being written" state; every loop is
// bounded by the probe window.  That is why born and tag are read only in the second launch: between the CAS that claims a slot and
// the claimer's store of born there is a moment in which the slot's words disagree, and nobody looks.
//
// FULL.  A thread that finds neither its key nor an empty slot in the window drops its index.  All indices of a call with one key
// share that fate: had any thread placed the key in slot s of the (shared) window, every walk that reaches s afterwards reads the key
// there (the CAS, or a plain load of a non-zero word), and a walk that passed s BEFORE saw another key in it -- which would still be
// there, so nobody could have placed ours.  Either all walks of a key end at its slot, or none finds one.  (The indices a
// wavefront's leader walks for share its fate by construction.)
//
// THE EPOCH lives in device memory, not in the kernel arguments: a captured graph replays its arguments frozen, and an epoch passed
// by value would make every replay the same call.  Two control words, so that no kernel reads a word it also writes: the first
// launch reads ctrl[1], uses e = ctrl[1] + 1 and one thread writes ctrl[0] = e; the second reads ctrl[0] and one thread writes
// ctrl[1] = ctrl[0].
//
// Entries and drops are counted with one atomic per wavefront (ballot + popcount), not one per lane.  Equal keys inside a wavefront
// are MERGED before they go to memory (key_place_kernel): a search level is full of duplicates, and unmerged every index sent two
// atomics to its slot's words, which ran at the rate ONE word takes them -- about 65 a microsecond, 1 ms for C4's 65 536 keys.
// profiles/key_table.txt has the worst case with and without the merge.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mgx_host.h"
#include "mgx_key_table.h"

namespace {

using namespace mgx;

constexpr int kKeyTableThreads = 256;          // one index per thread

struct KeyTableArgs {
    int64_t n;
    uint64_t mask;                             // capacity - 1
    uint32_t window, flags;
    MgxKeyTable t;
    const int64_t *keys;
    int64_t *entry, *first;
    uint8_t *is_new;
    int32_t *visits;
};

__global__ __launch_bounds__(kKeyTableThreads) void key_place_kernel(const KeyTableArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kKeyTableThreads + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t epoch = a.t.ctrl[KEY_CTRL_DONE] + 1u;           // (nobody writes that word in this launch)
    if (i == 0) a.t.ctrl[KEY_CTRL_CALL] = epoch;
    const bool active = i < a.n;
    const uint64_t k = active ? key_canon((uint64_t)a.keys[i]) : 0;
    // Equal keys of the wavefront meet before they go to memory: the lowest lane that holds a key -- the smallest index, since the
    // index grows with the lane -- leads; it walks and tags for all of them and counts them in one add.  One round per distinct key
    // of the wavefront, each a broadcast, a compare and a ballot.
    int leader = lane;
    uint32_t share = 1;
    for (unsigned long long todo = __ballot(active); todo;) {
        const int first = __ffsll(todo) - 1;
        const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)k, first), hi = __builtin_amdgcn_readlane((uint32_t)(k >> 32), first);
        const unsigned long long same = __ballot(active && k == (((uint64_t)hi << 32) | lo));
        if (active && k == (((uint64_t)hi << 32) | lo)) {
            leader = first;
            share = (uint32_t)__popcll(same);
        }
        todo &= ~same;
    }
    bool claimed = false;
    int64_t s = KEY_ABSENT;
    if (active && leader == lane) {
        const uint64_t home = key_home(k, a.mask + 1);
        for (uint32_t p = 0; p < a.window; ++p) {
            const uint64_t slot = (home + p) & a.mask;
            uint64_t cur = a.t.keys[slot];                         // plain: may be a stale "empty", never a stale key (see above)
            if (cur == 0) {
                cur = atomicCAS(reinterpret_cast<unsigned long long *>(a.t.keys + slot), 0ull, (unsigned long long)k);
                if (cur == 0) { claimed = true; cur = k; }
            }
            if (cur == k) { s = (int64_t)slot; break; }
        }
        if (s >= 0) {
            if (claimed) a.t.born[s] = epoch;
            atomicMax(reinterpret_cast<unsigned long long *>(a.t.tag + s), (unsigned long long)key_tag(epoch, (uint32_t)i));
            if (!(a.flags & MGX_KEY_NO_COUNT)) atomicAdd(a.t.visits + s, share);
        }
    }
    s = (int64_t)__shfl((int)s, leader);                            // (a slot is below 2^30, KEY_ABSENT is -1: 32 bits carry both)
    if (active) a.entry[i] = s;
    const unsigned long long placed = __ballot(claimed), lost = __ballot(active && s < 0);
    if (lane == 0) {
        if (placed) atomicAdd(a.t.ctrl + MGX_KEY_CTRL_ENTRIES, (uint32_t)__popcll(placed));
        if (lost) atomicAdd(a.t.ctrl + MGX_KEY_CTRL_DROPPED, (uint32_t)__popcll(lost));
    }
}

__global__ __launch_bounds__(kKeyTableThreads) void key_report_kernel(const KeyTableArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kKeyTableThreads + threadIdx.x;
    const uint32_t epoch = a.t.ctrl[KEY_CTRL_CALL];                // (nobody writes that word in this launch)
    if (i == 0) a.t.ctrl[KEY_CTRL_DONE] = epoch;
    if (i >= a.n) return;
    const int64_t s = a.entry[i];
    if (s < 0) {
        if (a.is_new) a.is_new[i] = 0;
        if (a.first) a.first[i] = KEY_ABSENT;
        if (a.visits) a.visits[i] = 0;
        return;
    }
    const uint64_t tag = a.t.tag[s];
    if (a.is_new) a.is_new[i] = key_is_new(a.t.born[s], tag, epoch, (uint32_t)i) ? 1 : 0;
    if (a.first) a.first[i] = (int64_t)key_tag_index(tag);
    if (a.visits) a.visits[i] = (int32_t)a.t.visits[s];
}

__global__ __launch_bounds__(kKeyTableThreads) void key_lookup_kernel(const KeyTableArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kKeyTableThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t k = key_canon((uint64_t)a.keys[i]), home = key_home(k, a.mask + 1);
    int64_t s = KEY_ABSENT;
    for (uint32_t p = 0; p < a.window; ++p) {
        const uint64_t slot = (home + p) & a.mask, cur = a.t.keys[slot];
        if (cur == k) { s = (int64_t)slot; break; }
        if (cur == 0) break;                                       // the invariant: the key would sit here or before
    }
    a.entry[i] = s;
    if (a.visits) a.visits[i] = s >= 0 ? (int32_t)a.t.visits[s] : 0;
}

// the checks the two entry points share, in the header's order; MGX_OK with *blocks == 0 means "nothing to launch"
int key_table_check(const MgxKeyTable *t, int64_t n, uint32_t flags, uint32_t known_flags, const int64_t *keys, const int64_t *entry,
                    const int64_t *first, const int32_t *visits, int64_t *blocks) {
    *blocks = 0;
    if (!t || !key_valid_capacity(t->capacity) || n < 0 || (flags & ~known_flags)) return MGX_ERR_INVALID_ARGUMENT;
    if (n == 0) return MGX_OK;
    if (!t->keys || !t->tag || !t->born || !t->visits || !t->ctrl || !keys || !entry) return MGX_ERR_INVALID_ARGUMENT;
    if (misaligned(t->keys, 8) || misaligned(t->tag, 8) || misaligned(t->born, 4) || misaligned(t->visits, 4) || misaligned(t->ctrl, 4)
        || misaligned(keys, 8) || misaligned(entry, 8) || misaligned(first, 8) || misaligned(visits, 4))
        return MGX_ERR_INVALID_ARGUMENT;
    if (n > (int64_t)INT_MAX) return MGX_ERR_UNSUPPORTED;         // (an index rides in the tag's low word)
    *blocks = (n + kKeyTableThreads - 1) / kKeyTableThreads;
    if (*blocks > INT_MAX) return MGX_ERR_UNSUPPORTED;
    return MGX_OK;
}

}  // namespace

extern "C" {

int mgx_key_insert(const MgxKeyTable *table, int64_t n, const int64_t *keys, uint32_t flags, int64_t *entry, uint8_t *is_new,
                   int64_t *first, int32_t *visits, void *stream) {
    int64_t blocks;
    const int rc = key_table_check(table, n, flags, MGX_KEY_NO_COUNT, keys, entry, first, visits, &blocks);
    if (rc != MGX_OK || blocks == 0) return rc;
    const KeyTableArgs args{n, (uint64_t)table->capacity - 1, key_window((uint64_t)table->capacity), flags, *table, keys, entry, first,
                            is_new, visits};
    hipLaunchKernelGGL(key_place_kernel, dim3((unsigned)blocks), dim3(kKeyTableThreads), 0, static_cast<hipStream_t>(stream), args);
    const int placed = finish_launch();
    if (placed != MGX_OK) return placed;
    hipLaunchKernelGGL(key_report_kernel, dim3((unsigned)blocks), dim3(kKeyTableThreads), 0, static_cast<hipStream_t>(stream), args);
    return finish_launch();
}

int mgx_key_lookup(const MgxKeyTable *table, int64_t n, const int64_t *keys, int64_t *entry, int32_t *visits, void *stream) {
    int64_t blocks;
    const int rc = key_table_check(table, n, 0, 0, keys, entry, nullptr, visits, &blocks);
    if (rc != MGX_OK || blocks == 0) return rc;
    const KeyTableArgs args{n, (uint64_t)table->capacity - 1, key_window((uint64_t)table->capacity), 0, *table, keys, entry, nullptr,
                            nullptr, visits};
    hipLaunchKernelGGL(key_lookup_kernel, dim3((unsigned)blocks), dim3(kKeyTableThreads), 0, static_cast<hipStream_t>(stream), args);
    return finish_launch();
}

}  // extern "C"
