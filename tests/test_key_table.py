"""The device key tables (include/mgx.h "KEY TABLES") without a GPU.

THE RULE is held to ONE reference: `ModelTable`, a dict-based NumPy / Python model of sequential insertion (the reference project
has no such notion).  csrc/mgx_key_table.h -- the statement the kernels are compiled from: the canonical key, `home`, the tag word,
and the serial insert and lookup over host arrays -- is built by g++ into a program of its own with its own main(), plain and under
ASan / UBSan, and run on case files written here; every output is compared with the model, `entry` exactly, since serial placement is
deterministic.  Nothing of it is loaded into Python.  The Python layer (`KeyTable`, `BatchedMultiGridEnv.key_table`) runs through
`KeyTableModel`, a launcher over the table's tensors, and examples/table_search.py through an oracle launcher plus that class.
tests/test_key_table_gpu.py holds the kernels to the same model."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import multigrid_amd
from multigrid_amd import EnvSpec, KeyInsert, KeyLookup, KeyTable, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK64 = (1 << 64) - 1
NO_COUNT = _lib.KEY_NO_COUNT
MAX_PROBE = 1024
TOP = -(1 << 63)                                          # a key with only the top bit set
#: the seeds of the random cases: the model drops nothing for any of them (test_the_random_cases_are_not_hollow)
SEEDS = (1, 2, 3)
CAPACITIES = (64, 128, 4096)


# ---- the rule in Python ------------------------------------------------------------------------------------------------------------

def mix(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def canon(k: int) -> int:
    """a key as the table holds it: unsigned, and 0 -> 1"""
    return (int(k) & MASK64) or 1


def home(k: int, capacity: int) -> int:
    return mix(canon(k)) & (capacity - 1)


def window(capacity: int) -> int:
    return min(capacity, MAX_PROBE)


def homes_np(keys: np.ndarray, capacity: int) -> np.ndarray:
    """`home` of an int64 / uint64 array, vectorised (mod 2^64 arithmetic of uint64)"""
    x = keys.astype(np.int64).view(np.uint64).copy()
    x[x == 0] = 1
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x & np.uint64(capacity - 1)).astype(np.int64)


def keys_with_home(capacity: int, target: int, count: int, start: int = 2) -> list:
    """the first `count` integers >= start whose home is `target`: how the tests construct collisions"""
    out, lo = [], start
    while len(out) < count:
        cand = np.arange(lo, lo + 65536, dtype=np.int64)
        out += cand[homes_np(cand, capacity) == target].tolist()
        lo += 65536
    return out[:count]


class ModelTable:
    """THE RULE: keys inserted one after another in index order.  `index` maps a canonical key to [slot, visits]."""

    def __init__(self, capacity: int):
        self.capacity, self.slots, self.index = capacity, [0] * capacity, {}
        self.entries = self.dropped = self.calls = 0
        self.longest_chain, self.wrapped = 1, False

    def _place(self, c: int):
        h = home(c, self.capacity)
        for p in range(window(self.capacity)):
            s = (h + p) & (self.capacity - 1)
            if self.slots[s] == 0:
                self.slots[s] = c
                self.longest_chain = max(self.longest_chain, p + 1)
                self.wrapped |= h + p >= self.capacity
                return s
            assert self.slots[s] != c
        return None

    def insert(self, keys, count=True):
        """(entry, is_new, first, visits) as int64 / bool / int64 / int32 arrays of the flattened keys"""
        keys = np.asarray(keys, dtype=np.int64).reshape(-1)
        n = keys.size
        entry, is_new = np.full(n, -1, np.int64), np.zeros(n, bool)
        first, visits, first_of = np.full(n, -1, np.int64), np.zeros(n, np.int32), {}
        self.calls += 1
        for i, k in enumerate(keys.tolist()):
            c = canon(k)
            rec, new = self.index.get(c), False
            if rec is None:
                s = self._place(c)
                if s is None:
                    self.dropped += 1
                    continue
                rec, new = [s, 0], True
                self.index[c] = rec
                self.entries += 1
            first_of.setdefault(c, i)
            rec[1] += int(count)
            entry[i], is_new[i], first[i] = rec[0], new, first_of[c]
        for i, k in enumerate(keys.tolist()):                                 # the count AFTER the call
            if entry[i] >= 0:
                visits[i] = self.index[canon(k)][1]
        return entry, is_new, first, visits

    def lookup(self, keys):
        keys = np.asarray(keys, dtype=np.int64).reshape(-1)
        recs = [self.index.get(canon(k)) for k in keys.tolist()]
        return (np.array([r[0] if r else -1 for r in recs], np.int64), np.array([r[1] if r else 0 for r in recs], np.int32))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def random_case(capacity: int, seed: int):
    """A list of calls ("insert", keys, flags) / ("lookup", keys) on one table that ends at a load of a half: three inserts (the
    second without counting) and two lookups.  The pool is random 64-bit keys plus the special ones: 0 and 1 (one entry), the top
    bit, three keys whose home is the table's last slot (their chain wraps) and three that share a home in the middle."""
    r = np.random.default_rng(1000 * capacity + seed)
    special = [0, 1, TOP, TOP + 5] + keys_with_home(capacity, capacity - 1, 3) + keys_with_home(capacity, capacity // 2, 3)
    pool = np.array(special + r.integers(-(1 << 63), (1 << 63) - 1, size=capacity // 2 + 1 - len(special), dtype=np.int64).tolist(), np.int64)
    assert len({canon(k) for k in pool.tolist()}) == capacity // 2                  # (0 and 1 are one key)
    rest = pool[len(special):]
    third = len(rest) // 3
    a = np.concatenate([pool[:len(special)], rest[:third], r.choice(rest[:third], size=third)])
    b = np.concatenate([rest[third // 2:2 * third], r.choice(pool, size=third)])
    c = np.concatenate([pool, r.choice(pool, size=third)])
    absent = r.integers(-(1 << 63), (1 << 63) - 1, size=third + 3, dtype=np.int64)
    for arr in (a, b, c):
        r.shuffle(arr)
    return [("insert", a, 0), ("lookup", np.concatenate([pool[:6], absent, rest[:third]])), ("insert", b, NO_COUNT), ("insert", c, 0),
            ("lookup", np.concatenate([absent, pool]))]


def run_model(capacity, calls):
    """the model's answers to a case: per call a dict of its outputs and the counters after it"""
    m, out = ModelTable(capacity), []
    for call in calls:
        if call[0] == "insert":
            entry, is_new, first, visits = m.insert(call[1], count=not call[2] & NO_COUNT)
            out.append(dict(entry=entry, is_new=is_new, first=first, visits=visits))
        else:
            entry, visits = m.lookup(call[1])
            out.append(dict(entry=entry, visits=visits))
        out[-1].update(entries=m.entries, dropped=m.dropped, calls=m.calls)
    return m, out


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_the_random_cases_are_not_hollow(capacity):
    """on the model alone, for the seeds 1, 2, 3: nothing is dropped at load 0.5, and every case holds keys new to the table, keys
    already in it, duplicates within a call, probe chains longer than 1 and a chain that wraps the table's end"""
    for seed in SEEDS:
        calls = random_case(capacity, seed)
        m, res = run_model(capacity, calls)
        assert m.dropped == 0 and m.entries == capacity // 2, (seed, m.dropped, m.entries)
        assert m.longest_chain > 1 and m.wrapped, (seed, m.longest_chain, m.wrapped)
        for idx in (2, 3):                                                    # the later inserts: all three kinds of index
            r, n = res[idx], len(calls[idx][1])
            known = ~r["is_new"] & (r["first"] == np.arange(n))               # first of its key in the call, and not new
            assert r["is_new"].any() and known.any() and (r["first"] != np.arange(n)).any(), (seed, idx)
        assert (res[1]["entry"] < 0).any() and (res[1]["entry"] >= 0).any() and (res[4]["entry"] >= 0).sum() == capacity // 2 + 1
        assert res[0]["visits"].max() > 1 and (res[3]["visits"] > res[2]["visits"].min()).any()


# ---- csrc/mgx_key_table.h, built by g++ into a program of its own --------------------------------------------------------------------

HOST_MAIN = r"""
// reads i64 words: capacity, calls, with_table (0: only `homes` calls follow, no table is allocated); per call: op (0 insert, 1 lookup, 2 homes), n, flags, want (bit 0 is_new, 1 first, 2 visits),
// keys[n].  Every output is allocated at its exact size, so that a sanitized build sees a write past it.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mgx_key_table.h"

template <typename T> static void line(const char *name, const std::vector<T> &v, bool have) {
    std::printf("%s", name);
    if (!have) std::printf(" -");
    else for (const T &x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> w;
    int64_t x;
    while (std::fread(&x, 8, 1, f) == 1) w.push_back(x);
    std::fclose(f);
    size_t at = 0;
    const int64_t cap = w[at++], calls = w[at++], slots = w[at++] ? cap : 0;
    if (!mgx::key_valid_capacity(cap)) { std::printf("invalid capacity\n"); return 0; }
    std::vector<uint64_t> keys(slots, 0), tag(slots, 0);
    std::vector<uint32_t> born(slots, 0), visits(slots, 0), ctrl(MGX_KEY_CTRL_WORDS, 0);
    const MgxKeyTable t{cap, keys.data(), tag.data(), born.data(), visits.data(), ctrl.data()};
    for (int64_t c = 0; c < calls; ++c) {
        const int64_t op = w[at++], n = w[at++], flags = w[at++], want = w[at++];
        const int64_t *in = w.data() + at;
        at += (size_t)n;
        std::vector<int64_t> entry(n, -7), first(n, -7);
        std::vector<uint8_t> is_new(n, 7);
        std::vector<int32_t> vis(n, -7);
        if (op == 0) {
            mgx::key_insert_host(t, n, in, (uint32_t)flags, entry.data(), (want & 1) ? is_new.data() : nullptr,
                                 (want & 2) ? first.data() : nullptr, (want & 4) ? vis.data() : nullptr);
            line("entry", entry, true); line("is_new", is_new, want & 1); line("first", first, want & 2); line("visits", vis, want & 4);
        } else if (op == 1) {
            mgx::key_lookup_host(t, n, in, entry.data(), (want & 4) ? vis.data() : nullptr);
            line("entry", entry, true); line("visits", vis, want & 4);
        } else {
            for (int64_t i = 0; i < n; ++i) entry[i] = (int64_t)mgx::key_home(mgx::key_canon((uint64_t)in[i]), (uint64_t)cap);
            line("home", entry, true);
            std::printf("window %u tag %llu index %u\n", mgx::key_window((uint64_t)cap), (unsigned long long)mgx::key_tag(3u, 5u),
                        mgx::key_tag_index(mgx::key_tag(3u, 5u)));
        }
        line("ctrl", ctrl, true);
    }
    std::vector<int64_t> held(slots);
    for (int64_t s = 0; s < slots; ++s) held[s] = (int64_t)keys[s];
    line("keys", held, true);
    return 0;
}
"""


def _i64(*values) -> bytes:
    return np.array(values, dtype=np.int64).tobytes()


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no C++ compiler"
    d = tmp_path_factory.mktemp("key_table_host")
    src = d / "key_table_host.cpp"
    src.write_text(HOST_MAIN)
    inc = ["-I", os.path.join(ROOT, "multigrid_amd", "csrc")]
    exes = {"plain": str(d / "plain"), "sanitized": str(d / "sanitized")}
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-Werror", *inc, str(src), "-o", exes["plain"]])
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           *inc, str(src), "-o", exes["sanitized"]])

    def run(which, payload: bytes):
        path = d / f"input_{which}.bin"
        path.write_bytes(payload)
        p = subprocess.run([exes[which], str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        return [ln for ln in p.stdout.split("\n") if ln]
    return run


def payload_of(capacity, calls, want=7) -> bytes:
    out = _i64(capacity, len(calls), int(any(c[0] != "home" for c in calls)))
    for call in calls:
        keys = np.asarray(call[1], dtype=np.int64).reshape(-1)
        op = {"insert": 0, "lookup": 1, "home": 2}[call[0]]
        out += _i64(op, keys.size, call[2] if op == 0 else 0, want) + keys.tobytes()
    return out


def lines_of(capacity, calls, want=7):
    """what the host program must print for a case, made from the model"""
    m, res = run_model(capacity, calls)
    fmt = lambda name, v, have=True: name + (" " + " ".join(str(int(x)) for x in v) if have and len(v) else ("" if have else " -"))
    out = []
    for call, r in zip(calls, res):
        out.append(fmt("entry", r["entry"]))
        if call[0] == "insert":
            out += [fmt("is_new", r["is_new"], want & 1), fmt("first", r["first"], want & 2)]
        out.append(fmt("visits", r["visits"], want & 4))
        out.append(f"ctrl {r['calls']} {r['calls']} {r['entries']} {r['dropped']} 0 0 0 0")       # (both epoch words: the inserts so far)
    out.append(fmt("keys", np.array(m.slots, dtype=np.uint64).view(np.int64)))
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
@pytest.mark.parametrize("capacity", CAPACITIES)
def test_the_header_program_equals_the_model(host_programs, capacity, which):
    for seed in SEEDS:
        calls = random_case(capacity, seed)
        for want in ((7, 0, 2) if seed == SEEDS[0] else (7,)):                # (every nullable output left out once)
            got = host_programs(which, payload_of(capacity, calls, want))
            assert got == lines_of(capacity, calls, want), (capacity, seed, want)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_header_program_on_full_tables_and_special_keys(host_programs, which):
    """serial and therefore deterministic: a table of 64 filled exactly drops nothing; new keys then are all dropped, the old ones
    found; 96 distinct keys into an empty table place the first 64; keys 0 and 1 are one entry; an empty call"""
    r = np.random.default_rng(7)
    keys = r.permutation(np.arange(1000, 1096, dtype=np.int64))
    cases = [(64, [("insert", keys[:64], 0), ("insert", np.concatenate([keys[60:70], keys[:4]]), 0), ("lookup", keys)]),
             (64, [("insert", keys, 0), ("lookup", keys), ("insert", keys[::-1].copy(), NO_COUNT)]),
             (64, [("insert", np.array([0, 1, 1, 0, TOP, -1], np.int64), 0), ("lookup", np.array([1, 0, 2, TOP], np.int64)),
                   ("insert", np.zeros(0, np.int64), 0), ("lookup", np.zeros(0, np.int64))]),
             (4096, [("insert", np.array(keys_with_home(4096, 4095, 1030), np.int64), 0)])]     # a window of 1024 in a larger table
    for capacity, calls in cases:
        assert host_programs(which, payload_of(capacity, calls)) == lines_of(capacity, calls), capacity
    m, res = run_model(*cases[0])
    assert res[0]["dropped"] == 0 and res[1]["dropped"] == 6 and res[1]["entry"].tolist()[:4] == [res[0]["entry"][i] for i in range(60, 64)]
    assert (res[1]["entry"][4:10] == -1).all() and (res[1]["first"][4:10] == -1).all() and (res[1]["visits"][4:10] == 0).all()
    m, res = run_model(*cases[1])
    assert res[0]["dropped"] == 32 and (res[0]["entry"][:64] >= 0).all() and (res[0]["entry"][64:] == -1).all() and res[2]["dropped"] == 64
    m, res = run_model(*cases[2])
    assert res[0]["entry"][0] == res[0]["entry"][1] == res[0]["entry"][2] and res[0]["visits"][:4].tolist() == [4] * 4 and m.entries == 3
    m, res = run_model(*cases[3])
    assert res[0]["dropped"] == 6 and m.entries == 1024 and m.wrapped and m.longest_chain == 1024


def test_the_python_home_is_the_headers(host_programs):
    """the restatement of `home` with which the GPU tests construct their collisions"""
    r = np.random.default_rng(11)
    keys = np.concatenate([np.array([0, 1, 2, -1, TOP, TOP + 1], np.int64), r.integers(-(1 << 63), (1 << 63) - 1, size=200, dtype=np.int64)])
    for capacity in (64, 4096, 1 << 30):
        got = host_programs("plain", payload_of(capacity, [("home", keys, 0)]))
        want = [home(k, capacity) for k in keys.tolist()]
        assert got[0] == "home " + " ".join(map(str, want)) and want == homes_np(keys, capacity).tolist()
        assert got[-1] == "keys" and got[1] == f"window {min(capacity, 1024)} tag {(3 << 32) | (0xFFFFFFFF - 5)} index 5"
    assert home(0, 64) == home(1, 64) and mix(0) == 0xE220A8397B1DCDAF
    for capacity, target in ((64, 63), (4096, 4095), (128, 17)):
        found = keys_with_home(capacity, target, 5)
        assert len(set(found)) == 5 and all(home(k, capacity) == target for k in found)
    for capacity in (0, 32, 96, 1 << 31):
        assert host_programs("plain", payload_of(capacity, [])) == ["invalid capacity"]


# ---- the Python layer over a launcher that works on the table's tensors -------------------------------------------------------------

class KeyTableModel:
    """`key_insert` / `key_lookup` of a backend, on CPU tensors: the serial statement over the table's own arrays (so that entries(),
    occupied(), state_dict() and clear() see a real table), refusing what the entry points refuse.  A mixin: it keeps no state."""

    @staticmethod
    def _arrays(table):
        cap = table["capacity"]
        a = {m: table[m].numpy() for m in ("keys", "tag", "born", "visits", "ctrl")}
        assert a["keys"].shape == a["tag"].shape == a["born"].shape == a["visits"].shape == (cap,) and a["ctrl"].shape == (8,)
        assert a["keys"].dtype == a["tag"].dtype == np.int64 and a["born"].dtype == a["visits"].dtype == a["ctrl"].dtype == np.int32
        return cap, a

    def key_insert(self, table, n, keys, flags, entry, is_new, first, visits):
        cap, a = self._arrays(table)
        if flags & ~NO_COUNT or n >= 2 ** 31:
            raise _lib.MgxError(_lib.ERR_INVALID_ARGUMENT if flags & ~NO_COUNT else _lib.ERR_UNSUPPORTED, "mgx_key_insert")
        assert keys.dtype is torch.int64 and keys.numel() == n and entry.dtype is torch.int64 and entry.shape == keys.shape
        assert is_new is None or (is_new.dtype is torch.bool and is_new.shape == keys.shape)
        assert first is None or (first.dtype is torch.int64 and first.shape == keys.shape)
        assert visits is None or (visits.dtype is torch.int32 and visits.shape == keys.shape)
        held, ctrl = a["keys"].view(np.uint64), a["ctrl"]
        epoch = int(ctrl[1]) + 1
        ctrl[0] = epoch
        flat, e = keys.reshape(-1).tolist(), entry.view(-1)
        for i, k in enumerate(flat):
            c, s = canon(k), -1
            h = home(c, cap)
            for p in range(window(cap)):
                slot = (h + p) & (cap - 1)
                if held[slot] == 0:
                    held[slot], a["born"][slot] = c, epoch
                    ctrl[2] += 1
                if held[slot] == c:
                    s = slot
                    break
            e[i] = s
            if s < 0:
                ctrl[3] += 1
                continue
            a["tag"][s] = max(int(a["tag"][s]), (epoch << 32) | (0xFFFFFFFF - i))
            a["visits"][s] += 0 if flags & NO_COUNT else 1
        for i in range(n):
            s = int(e[i])
            if is_new is not None:
                is_new.view(-1)[i] = s >= 0 and int(a["born"][s]) == epoch and 0xFFFFFFFF - (int(a["tag"][s]) & 0xFFFFFFFF) == i
            if first is not None:
                first.view(-1)[i] = 0xFFFFFFFF - (int(a["tag"][s]) & 0xFFFFFFFF) if s >= 0 else -1
            if visits is not None:
                visits.view(-1)[i] = int(a["visits"][s]) if s >= 0 else 0
        ctrl[1] = epoch

    def key_lookup(self, table, n, keys, entry, visits):
        cap, a = self._arrays(table)
        held = a["keys"].view(np.uint64)
        assert keys.dtype is torch.int64 and keys.numel() == n and entry.shape == keys.shape
        for i, k in enumerate(keys.reshape(-1).tolist()):
            c, s = canon(k), -1
            h = home(c, cap)
            for p in range(window(cap)):
                slot = (h + p) & (cap - 1)
                if held[slot] == c:
                    s = slot
                    break
                if held[slot] == 0:
                    break
            entry.view(-1)[i] = s
            if visits is not None:
                visits.view(-1)[i] = int(a["visits"][s]) if s >= 0 else 0


def cpu_table(capacity=64):
    return KeyTable(capacity, "cpu", backend=KeyTableModel())


def test_the_model_launcher_equals_the_model():
    """KeyTable over KeyTableModel against ModelTable, call by call, `entry` included (both place serially)"""
    for capacity in (64, 128):
        calls = random_case(capacity, SEEDS[0])
        t, (m, res) = cpu_table(capacity), run_model(capacity, calls)
        for call, r in zip(calls, res):
            keys = torch.from_numpy(call[1].copy())
            if call[0] == "insert":
                got = t.insert(keys, first=True, visits=True, count=not call[2])
                assert got.is_new.dtype is torch.bool and got.is_new.numpy().tolist() == r["is_new"].tolist()
                assert got.first.numpy().tolist() == r["first"].tolist()
            else:
                got = t.lookup(keys, visits=True)
            assert got.entry.numpy().tolist() == r["entry"].tolist() and got.visits.numpy().tolist() == r["visits"].tolist()
            assert (t.entries(), t.dropped()) == (r["entries"], r["dropped"])
        assert t.keys.numpy().view(np.uint64).tolist() == m.slots and t.occupied().tolist() == [s for s in range(capacity) if m.slots[s]]


def test_insert_and_lookup_shapes_outputs_and_out_reuse():
    t = cpu_table(128)
    assert multigrid_amd.KeyTable is KeyTable and "KeyTable" in multigrid_amd.__all__
    keys = torch.tensor([[5, 6, 5], [7, 5, 6]], dtype=torch.int64)            # obs_key()'s [B, A] goes in as it is
    res = t.insert(keys)
    assert isinstance(res, KeyInsert) and res.first is None and res.visits is None
    assert res.entry.shape == keys.shape and res.entry.dtype is torch.int64 and res.is_new.dtype is torch.bool
    assert res.is_new.tolist() == [[True, True, False], [True, False, False]]
    assert res.entry[0, 0] == res.entry[0, 2] == res.entry[1, 1] and len(set(res.entry.view(-1).tolist())) == 3
    full = t.insert(keys, first=True, visits=True)
    assert not full.is_new.any() and full.first.tolist() == [[0, 1, 0], [3, 0, 1]] and full.visits.tolist() == [[6, 4, 6], [2, 6, 4]]
    assert torch.equal(full.entry, res.entry)
    only = t.insert(keys, is_new=False, count=False)
    assert only.is_new is None and only.first is None and only.visits is None and torch.equal(only.entry, res.entry)
    again = t.insert(keys, first=True, visits=True, out=full)                 # out=: the same tensors, nothing allocated
    assert all(x is y for x, y in zip(again, full)) and again.visits.tolist() == [[9, 6, 9], [3, 9, 6]]
    part = t.insert(keys, out=full, count=False)                              # (fewer outputs than out= holds: the rest is not written)
    assert part.entry is full.entry and part.is_new is full.is_new and part.first is None and part.visits is None
    found = t.lookup(torch.tensor([7, 8, 5], dtype=torch.int64), visits=True)
    assert isinstance(found, KeyLookup) and found.entry.tolist() == [int(res.entry[1, 0]), -1, int(res.entry[0, 0])]
    assert found.visits.tolist() == [3, 0, 9] and t.lookup(keys).visits is None
    same = t.lookup(torch.tensor([5, 5, 9], dtype=torch.int64), visits=True, out=found)
    assert same.entry is found.entry and same.visits is found.visits and same.visits.tolist() == [9, 9, 0]
    empty = t.insert(torch.zeros((0, 2), dtype=torch.int64))
    assert empty.entry.shape == (0, 2) and t.entries() == 3 and t.dropped() == 0
    assert t.keys[t.occupied()].sort().values.tolist() == [5, 6, 7]


def test_arguments_are_refused_by_name():
    for capacity in (0, 63, 96, 32, 1 << 31, 64.0, True, None):
        with pytest.raises(ValueError, match="KeyTable: capacity must be a power of two"):
            KeyTable(capacity, "cpu", backend=KeyTableModel())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KeyTable(64, "cpu")
    t = cpu_table()
    good = torch.arange(2, 8, dtype=torch.int64)
    for bad in (good.to(torch.int32), good[::2], [1, 2], good.view(2, 3).t(), None):
        with pytest.raises(ValueError, match="insert: keys must be a contiguous int64 tensor on cpu"):
            t.insert(bad)
        with pytest.raises(ValueError, match="lookup: keys must be a contiguous int64 tensor on cpu"):
            t.lookup(bad)
    res = t.insert(good)
    with pytest.raises(ValueError, match="insert: out= holds no `first`"):
        t.insert(good, first=True, out=res)
    with pytest.raises(ValueError, match=r"insert: out=.entry must be a contiguous int64 tensor of shape \(3,\)"):
        t.insert(good[:3], out=res)
    with pytest.raises(ValueError, match="insert: out= must be a KeyInsert"):
        t.insert(good, out=res.entry)
    with pytest.raises(ValueError, match="insert: out=.is_new must be a contiguous bool"):
        t.insert(good, out=KeyInsert(res.entry, res.entry, None, None))
    with pytest.raises(ValueError, match="lookup: out= holds no tensor"):
        t.lookup(good, visits=True, out=t.lookup(good))
    with pytest.raises(ValueError, match="lookup: out= must be a KeyLookup"):
        t.lookup(good, out=res.entry)
    assert t.entries() == 6 and t.insert(good, visits=True).visits.tolist() == [2] * 6       # the refused calls inserted nothing


def test_check_errors_names_the_drops_and_starts_anew():
    t = cpu_table(64)
    res = t.insert(torch.arange(100, 196, dtype=torch.int64), first=True, visits=True)
    assert t.entries() == 64 and t.dropped() == 32 and (res.entry[64:] == -1).all() and not res.is_new[64:].any()
    assert (res.first[64:] == -1).all() and (res.visits[64:] == 0).all() and res.is_new[:64].all()
    with pytest.raises(ValueError, match=r"KeyTable: 32 inserted key\(s\) were dropped.*capacity 64, 64 entries"):
        t.check_errors()
    t.check_errors()                                                          # raises once
    assert t.dropped() == 0 and t.entries() == 64


def test_state_dict_round_trip_and_clear():
    t = cpu_table(64)
    keys = torch.tensor([3, 4, 3, 0], dtype=torch.int64)
    first = t.insert(keys, visits=True)
    state = t.state_dict()
    assert sorted(state) == ["born", "ctrl", "keys", "tag", "visits"] and all(torch.is_tensor(v) for v in state.values())
    assert state["keys"].data_ptr() != t.keys.data_ptr()
    t.insert(torch.tensor([9, 3], dtype=torch.int64))
    other = cpu_table(64)
    other.load_state_dict(state)
    assert other.entries() == 3 and torch.equal(other.lookup(keys).entry, first.entry)
    nxt = other.insert(torch.tensor([9, 3], dtype=torch.int64), first=True, visits=True)      # the epoch travels with the state
    assert nxt.is_new.tolist() == [True, False] and nxt.first.tolist() == [0, 1] and nxt.visits.tolist() == [1, 3]
    with pytest.raises(ValueError, match="load_state_dict: keys must be a int64 tensor of shape \\(128,\\)"):
        cpu_table(128).load_state_dict(state)
    with pytest.raises(ValueError, match="load_state_dict: expected the members"):
        other.load_state_dict({"keys": state["keys"]})
    other.clear()
    assert other.entries() == 0 and other.occupied().numel() == 0 and not other._buf.any()
    res = other.insert(keys, first=True, visits=True)                         # reuse: epochs and counts start at 1 again
    assert res.is_new.tolist() == [True, True, False, True] and res.visits.tolist() == [2, 1, 2, 1] and int(other.ctrl[1]) == 1
    assert other.lookup(torch.tensor([9], dtype=torch.int64)).entry.tolist() == [-1]
    # the arrays are views of one zero-filled buffer of 24 * capacity + 32 bytes, laid out as the header says
    assert t._buf.numel() * 8 == 24 * 64 + 32 and t.tag.data_ptr() == t.keys.data_ptr() + 8 * 64
    assert t.born.data_ptr() == t.keys.data_ptr() + 16 * 64 and t.visits.data_ptr() == t.born.data_ptr() + 4 * 64
    assert t.ctrl.data_ptr() == t.visits.data_ptr() + 4 * 64 and t.ctrl.shape == (8,)


def test_an_env_makes_tables_on_its_device_with_its_backend():
    from tests.test_env_snapshot import make_env
    from tests.test_state_key import KeyOracle

    class Oracle(KeyOracle, KeyTableModel):
        pass
    spec = EnvSpec(5, 5, 2, 3, max_steps=6)
    env = make_env("pool", B=7, spec=spec, backend=Oracle(spec))
    t = env.key_table(64)
    assert isinstance(t, KeyTable) and t.backend is env.backend and t.device == env.agents.device and t.capacity == 64
    keys = env.state_key()
    res = t.insert(keys, first=True)
    m = ModelTable(64)
    _, is_new, first, _ = m.insert(keys.numpy())
    assert res.is_new.tolist() == is_new.tolist() and res.first.tolist() == first.tolist() and t.entries() == m.entries
    snap = env.snapshot()
    assert not t.insert(snap.state_key(torch.tensor([6, 0]))).is_new.any()     # a snapshot's keys go into the same table
    with pytest.raises(ValueError, match="KeyTable: capacity"):
        env.key_table(100)


def test_the_example_chooses_what_the_torch_formulation_chooses():
    """examples/table_search.py with check=True on 1024 envs of C2 (Empty-16x16), one root, a beam of 8, through an oracle launcher
    plus the model launcher: at every level the table's new keys are the torch formulation's, and the search finds the goal at the
    depth examples/best_first.py finds it"""
    import importlib.util
    from multigrid_amd import workloads
    from tests.test_distance import DistOracle
    from tests.test_state_key import KeyOracle

    class SearchOracle(DistOracle, KeyOracle, KeyTableModel):
        pass
    mod_spec = importlib.util.spec_from_file_location("table_search", os.path.join(ROOT, "examples", "table_search.py"))
    mod = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(mod)
    out = mod.run("c2", roots=1, beam=8, depth=40, batch=1024, device="cpu", backend=SearchOracle(workloads.spec_of("c2")), capacity=4096,
                  check=True)
    assert out["found"] and out["depth"] == 27 and out["drops"] == 0 and out["checked"]
    assert out["table_entries"] == 1 + sum(out["new_per_level"]) and len(out["new_per_level"]) == 26 and min(out["new_per_level"]) > 0
    assert out["nodes_expanded"] < 27 * 8
    with pytest.raises(ValueError, match="no goal cell"):
        mod.run("c3", batch=64, device="cpu", backend=SearchOracle(workloads.spec_of("c3")))


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------------

def test_c_abi_argument_validation():
    """the return codes of both entry points in the header's order; no call gets as far as a launch"""
    L = _lib.lib()
    INV, UNS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
    p, big = 4096, 2 ** 31                                # (never dereferenced: every call returns before a launch)
    members = ("keys", "tag", "born", "visits", "ctrl")
    table = lambda capacity=64, **kw: _lib.MgxKeyTableC(capacity, *[kw.get(m, p) for m in members])
    ref = lambda x: C.byref(x) if x is not None else None

    def ins(t, n, keys=p, flags=0, entry=p, is_new=p + 1, first=p, visits=p + 4):
        return L.mgx_key_insert(ref(t), n, keys, flags, entry, is_new, first, visits, None)

    def look(t, n, keys=p, entry=p, visits=p + 4):
        return L.mgx_key_lookup(ref(t), n, keys, entry, visits, None)
    t = table()
    # first: the table, its capacity, n, the flags -- before n == 0 is answered
    for n in (big, 0):
        assert ins(None, n) == INV and look(None, n) == INV
        for capacity in (0, 1, 32, 63, 96, -64, 2 ** 31, 2 ** 30 + 1):
            assert ins(table(capacity), n) == INV and look(table(capacity), n) == INV, capacity
        for flags in (2, 3, 0x80000000):
            assert ins(t, n, flags=flags) == INV
    assert ins(t, -1) == INV and look(t, -1) == INV
    # then n == 0: nothing is looked at any more
    assert ins(t, 0) == 0 and look(t, 0) == 0 and ins(table(2 ** 30), 0, flags=1) == 0
    assert ins(table(64, keys=None, ctrl=None), 0, None, 0, None, None, None, None) == 0 and look(table(64, tag=3), 0, None, None, None) == 0
    # then the required pointers and the alignments -- before the size is looked at
    for n in (4, big):
        for m in members:
            assert ins(table(**{m: None}), n) == INV and look(table(**{m: None}), n) == INV, m
        for m, off in (("keys", 4), ("tag", 4), ("born", 2), ("visits", 2), ("ctrl", 2)):
            assert ins(table(**{m: p + off}), n) == INV and look(table(**{m: p + off}), n) == INV, m
        assert ins(t, n, keys=None) == INV and ins(t, n, entry=None) == INV and look(t, n, keys=None) == INV and look(t, n, entry=None) == INV
        assert ins(t, n, keys=p + 4) == INV and ins(t, n, entry=p + 4) == INV and ins(t, n, first=p + 4) == INV and ins(t, n, visits=p + 2) == INV
        assert look(t, n, keys=p + 4) == INV and look(t, n, entry=p + 4) == INV and look(t, n, visits=p + 2) == INV
    # then the size: an index must fit the tag's low word
    assert ins(t, big) == UNS and look(t, big) == UNS and ins(t, 2 ** 40, flags=1) == UNS
    assert ins(t, big, is_new=None, first=None, visits=None) == UNS and look(t, big, visits=None) == UNS     # (the nullable outputs)
    assert ins(table(2 ** 30), big) == UNS


def test_the_exports_are_the_headers_declarations():
    from tests.test_capi import declared_functions
    names = declared_functions()
    for name in ("mgx_key_insert", "mgx_key_lookup"):
        assert name in names and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    assert set(names) == set(_lib.EXPORTS) and _lib.lib().mgx_abi_version() == _lib.ABI_VERSION == 11
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "KEY TABLES" in hdr and "enum { MGX_KEY_NO_COUNT = 1 };" in hdr
    assert ("MGX_KEY_MAX_PROBE = 1024, MGX_KEY_MIN_CAPACITY = 64, MGX_KEY_MAX_CAPACITY = 1 << 30, MGX_KEY_CTRL_WORDS = 8,\n"
            "       MGX_KEY_CTRL_ENTRIES = 2, MGX_KEY_CTRL_DROPPED = 3") in hdr
    assert (_lib.KEY_NO_COUNT, _lib.KEY_MAX_PROBE, _lib.KEY_MIN_CAPACITY, _lib.KEY_MAX_CAPACITY, _lib.KEY_CTRL_WORDS, _lib.KEY_CTRL_ENTRIES,
            _lib.KEY_CTRL_DROPPED) == (1, 1024, 64, 1 << 30, 8, 2, 3) and MAX_PROBE == _lib.KEY_MAX_PROBE
    assert C.sizeof(_lib.MgxKeyTableC) == 48 and [f for f, _ in _lib.MgxKeyTableC._fields_] == ["capacity", "keys", "tag", "born", "visits", "ctrl"]
    from multigrid_amd import build
    assert any(u[0] == "mgx_key_table" for u in build.UNITS) and os.path.join(build.CSRC, "mgx_key_table.h") in build.DEPS
