// mgx_key_table.h -- the rule of the device key tables (include/mgx.h: "KEY TABLES"), stated once for both compilers: the kernels of
// mgx_key_table.hip canonicalise, place and tag with these functions, and g++ builds the same header into the stand-alone program of
// tests/test_key_table.py, which holds `key_insert_host` / `key_lookup_host` -- the serial statement over host arrays -- to a
// dict-based NumPy model of THE RULE.
//
// THE INVARIANT: entries are never removed, so a slot goes from empty (0) to one key exactly once and never changes again.  Every
// slot before a key's slot in its window therefore holds another key for good, and a walk may stop at the first empty slot.
#pragma once
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

constexpr int64_t KEY_ABSENT = -1;             // entry / first of a key that is not, or could not be, in the table
constexpr int KEY_CTRL_CALL = 0;               // ctrl[0]: the epoch of the insert whose first launch ran last
constexpr int KEY_CTRL_DONE = 1;               // ctrl[1]: the epoch of the last finished insert

// key 0 marks an empty slot: it is stored and answered as key 1
MGX_HD uint64_t key_canon(uint64_t k) { return k ? k : 1ull; }

// splitmix64 (the mixer of mgx_state_key.h): callers may pass keys that are not hash outputs
MGX_HD uint64_t key_table_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the first slot of the canonical key k's window; capacity is a power of two
MGX_HD uint64_t key_home(uint64_t k, uint64_t capacity) { return key_table_mix(k) & (capacity - 1); }
// the window's length: a key is looked for, and placed, in the slots (home + p) & (capacity - 1), p < key_window(capacity)
MGX_HD uint32_t key_window(uint64_t capacity) { return capacity < (uint64_t)MGX_KEY_MAX_PROBE ? (uint32_t)capacity : (uint32_t)MGX_KEY_MAX_PROBE; }

// The tag word of a slot: a later call beats every earlier one, and within a call the smallest index wins an atomic max.
MGX_HD uint64_t key_tag(uint32_t epoch, uint32_t i) { return ((uint64_t)epoch << 32) | (uint64_t)(0xFFFFFFFFu - i); }
MGX_HD uint32_t key_tag_index(uint64_t tag) { return 0xFFFFFFFFu - (uint32_t)tag; }
MGX_HD bool key_valid_capacity(int64_t c) {
    return c >= MGX_KEY_MIN_CAPACITY && c <= MGX_KEY_MAX_CAPACITY && (c & (c - 1)) == 0;
}

// what the second launch of an insert reads back for index i of the call `epoch`, whose key sits in slot s
MGX_HD bool key_is_new(uint32_t born, uint64_t tag, uint32_t epoch, uint32_t i) { return born == epoch && key_tag_index(tag) == i; }

// The serial statement: keys[0..n) one after another in index order.  Serial placement is deterministic, `entry` included.
inline void key_insert_host(const MgxKeyTable &t, int64_t n, const int64_t *keys, uint32_t flags, int64_t *entry, uint8_t *is_new,
                            int64_t *first, int32_t *visits) {
    const uint64_t cap = (uint64_t)t.capacity, mask = cap - 1;
    const uint32_t window = key_window(cap), epoch = t.ctrl[KEY_CTRL_DONE] + 1;
    t.ctrl[KEY_CTRL_CALL] = epoch;
    for (int64_t i = 0; i < n; ++i) {                              // the first launch
        const uint64_t k = key_canon((uint64_t)keys[i]), home = key_home(k, cap);
        int64_t s = KEY_ABSENT;
        for (uint32_t p = 0; p < window; ++p) {
            const uint64_t slot = (home + p) & mask;
            if (t.keys[slot] == 0) {
                t.keys[slot] = k;
                t.born[slot] = epoch;
                t.ctrl[MGX_KEY_CTRL_ENTRIES] += 1;
            }
            if (t.keys[slot] == k) { s = (int64_t)slot; break; }
        }
        entry[i] = s;
        if (s < 0) { t.ctrl[MGX_KEY_CTRL_DROPPED] += 1; continue; }
        const uint64_t tag = key_tag(epoch, (uint32_t)i);
        if (tag > t.tag[s]) t.tag[s] = tag;
        if (!(flags & MGX_KEY_NO_COUNT)) t.visits[s] += 1;
    }
    for (int64_t i = 0; i < n; ++i) {                              // the second launch
        const int64_t s = entry[i];
        if (is_new) is_new[i] = s >= 0 && key_is_new(t.born[s], t.tag[s], epoch, (uint32_t)i);
        if (first) first[i] = s >= 0 ? (int64_t)key_tag_index(t.tag[s]) : KEY_ABSENT;
        if (visits) visits[i] = s >= 0 ? (int32_t)t.visits[s] : 0;
    }
    t.ctrl[KEY_CTRL_DONE] = epoch;
}

inline void key_lookup_host(const MgxKeyTable &t, int64_t n, const int64_t *keys, int64_t *entry, int32_t *visits) {
    const uint64_t cap = (uint64_t)t.capacity, mask = cap - 1;
    const uint32_t window = key_window(cap);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t k = key_canon((uint64_t)keys[i]), home = key_home(k, cap);
        int64_t s = KEY_ABSENT;
        for (uint32_t p = 0; p < window; ++p) {
            const uint64_t slot = (home + p) & mask, cur = t.keys[slot];
            if (cur == k) { s = (int64_t)slot; break; }
            if (cur == 0) break;                                   // (the invariant: the key would sit here or before)
        }
        entry[i] = s;
        if (visits) visits[i] = s >= 0 ? (int32_t)t.visits[s] : 0;
    }
}

}  // namespace mgx
