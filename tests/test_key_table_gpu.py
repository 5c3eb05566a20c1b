"""The key-table kernels (csrc/mgx_key_table.hip) against the dict-based model of tests/test_key_table.py, on the device.  is_new,
first, visits, found / absent and the two counters are compared bit for bit; `entry` -- whose values depend on the order in which
threads arrive -- by its properties: in range, equal iff the keys are equal, `table.keys[entry]` the canonical key, and the same
from every lookup and every later insert.  Every output sits between guard words, and the keys are a view one element into a larger
allocation.

Which of these tests fail under which mutant of the kernels -- each mutant was built as a library of its own (every one of them
in bounds) and this file run against it on an MI355X:
  the epoch passed by value              test_a_captured_insert_is_a_new_call_at_every_replay (every replay is the same call: the
                                         keys are "new" again), test_special_keys_and_clear (a cleared table meets a later epoch)
  `first` from the claiming thread       23 of the 27 cases, among them test_every_key_equal_and_keys_spread_over_all_xcds and all
                                         of test_sizes from n = 63 on (the claimer is whoever arrives first, and a key that was
                                         already in the table has no claimer at all)
  a probe that does not wrap             test_chains_that_share_a_home_and_wrap, test_the_random_cases_of_the_cpu_tests,
                                         test_full_tables, two of test_sizes (keys whose home is near the end are dropped)
  a lookup that ignores empty slots      test_a_lookup_stops_at_the_first_empty_slot alone (a hand-made table that breaks the
                                         invariant: with the invariant intact that mutant is only slower)
  a lookup that stops at a foreign key   17 cases: test_chains_that_share_a_home_and_wrap, test_the_random_cases_of_the_cpu_tests,
                                         test_full_tables, most of test_sizes"""
import numpy as np
import pytest
import torch

from multigrid_amd import EnvSpec, KeyInsert, KeyLookup, KeyTable
from tests.test_key_table import SEEDS, TOP, KeyTableModel, ModelTable, canon, keys_with_home, random_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WG = 256                                                  # threads per workgroup of the three kernels: one index each
GUARD64, GUARD32, GUARD8 = -0x0123456789ABCDEF, -0x01234567, 0xAB


def guarded(n, dtype):
    """(the whole allocation, its middle n elements): an output between two guard words"""
    if dtype is torch.bool:
        full = torch.full((n + 2,), GUARD8, dtype=torch.uint8, device=DEV)
        return full, full[1:n + 1].view(torch.bool)
    full = torch.full((n + 2,), GUARD64 if dtype is torch.int64 else GUARD32, dtype=dtype, device=DEV)
    return full, full[1:n + 1]


def guards_hold(full):
    g = GUARD8 if full.dtype is torch.uint8 else (GUARD64 if full.dtype is torch.int64 else GUARD32)
    return int(full[0]) == g and int(full[-1]) == g


def on_device(keys):
    """the keys as a view one element into a larger allocation"""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1)
    full = torch.from_numpy(np.concatenate([[GUARD64], keys, [GUARD64]]).astype(np.int64)).to(DEV)
    return full[1:keys.size + 1]


class Pair:
    """a device table and the model beside it; `known` remembers every key's entry id, which must never change"""

    def __init__(self, capacity, table=None):
        self.t = table if table is not None else KeyTable(capacity, DEV)
        self.m, self.known, self.capacity = ModelTable(capacity), {}, capacity

    def _entries(self, keys, entry, placed):
        """the properties of `entry` at the indices the model placed / found, -1 elsewhere"""
        entry = entry.cpu().numpy()
        assert (entry[~placed] == -1).all()
        e, ck = entry[placed], [canon(k) for k in keys[placed].tolist()]
        assert ((e >= 0) & (e < self.capacity)).all()
        assert len(set(zip(ck, e.tolist()))) == len(set(ck)) == len(set(e.tolist()))              # equal iff the keys are equal
        held = self.t.keys[torch.from_numpy(e).to(DEV)].cpu().numpy().view(np.uint64).tolist()
        assert held == ck                                                                          # the slot holds the canonical key
        for c, s in zip(ck, e.tolist()):
            assert self.known.setdefault(c, s) == s                                                # the same in every later call

    def counters(self):
        assert (self.t.entries(), self.t.dropped()) == (self.m.entries, self.m.dropped)
        assert int(self.t.ctrl[0]) == int(self.t.ctrl[1]) and self.t.ctrl[4:].tolist() == [0] * 4

    def insert(self, keys, count=True, deterministic=True):
        keys = np.asarray(keys, dtype=np.int64).reshape(-1)
        n = keys.size
        outs = [guarded(n, dt) for dt in (torch.int64, torch.bool, torch.int64, torch.int32)]
        res = self.t.insert(on_device(keys), first=True, visits=True, count=count, out=KeyInsert(*[o[1] for o in outs]))
        want_entry, is_new, first, visits = self.m.insert(keys, count=count)
        torch.cuda.synchronize()
        assert all(guards_hold(o[0]) for o in outs)
        if deterministic:                                  # (when more new keys arrive than fit, WHICH are dropped is arrival order)
            assert res.is_new.cpu().numpy().tolist() == is_new.tolist()
            assert res.first.cpu().numpy().tolist() == first.tolist()
            assert res.visits.cpu().numpy().tolist() == visits.tolist()
            self._entries(keys, res.entry, want_entry >= 0)
        self.counters()
        return res

    def lookup(self, keys):
        keys = np.asarray(keys, dtype=np.int64).reshape(-1)
        outs = [guarded(keys.size, dt) for dt in (torch.int64, torch.int32)]
        res = self.t.lookup(on_device(keys), visits=True, out=KeyLookup(*[o[1] for o in outs]))
        want_entry, visits = self.m.lookup(keys)
        torch.cuda.synchronize()
        assert all(guards_hold(o[0]) for o in outs)
        assert res.visits.cpu().numpy().tolist() == visits.tolist()
        self._entries(keys, res.entry, want_entry >= 0)
        self.counters()
        return res


@pytest.mark.parametrize("n", [1, 63, 64, 65, WG + 1])
@pytest.mark.parametrize("capacity", [64, 128, 4096])
def test_sizes(capacity, n):
    """capacity 64 is the minimum, where the window is the whole table; n around a wavefront and one workgroup + 1"""
    r = np.random.default_rng(capacity + n)
    pool = r.integers(-(1 << 63), (1 << 63) - 1, size=min(capacity // 2, max(n, 2)), dtype=np.int64)
    p = Pair(capacity)
    p.insert(r.choice(pool[:max(1, len(pool) // 2)], size=n))
    p.insert(r.choice(pool, size=n))
    p.lookup(np.concatenate([pool, r.integers(-(1 << 63), (1 << 63) - 1, size=5, dtype=np.int64)])[:max(n, 6)])
    assert p.m.dropped == 0


@pytest.mark.parametrize("capacity", [64, 128, 4096])
def test_the_random_cases_of_the_cpu_tests(capacity):
    """three inserts (the second with MGX_KEY_NO_COUNT) and two lookups into one table: new keys, known keys, duplicates, chains
    longer than 1, a chain that wraps, keys 0 and 1, keys with the top bit"""
    p = Pair(capacity)
    for call in random_case(capacity, SEEDS[0]):
        if call[0] == "insert":
            p.insert(call[1], count=not call[2])
        else:
            p.lookup(call[1])
    assert p.m.wrapped and p.m.longest_chain > 1 and p.m.dropped == 0 and p.t.entries() == capacity // 2


def test_every_key_equal_and_keys_spread_over_all_xcds():
    """the contention cases: one key at one workgroup + 1 indices; 32 keys as i % 32 over 16 workgroups, so that duplicates of every
    key sit in workgroups on all eight XCDs -- what catches a read trusted across XCDs inside the first launch"""
    p = Pair(128)
    res = p.insert(np.full(WG + 1, 77, np.int64))
    assert res.is_new.sum().item() == 1 and bool(res.is_new[0]) and (res.first == 0).all() and (res.visits == WG + 1).all()
    assert p.t.entries() == 1
    res = p.insert(np.full(WG + 1, 77, np.int64))
    assert not res.is_new.any() and (res.visits == 2 * (WG + 1)).all()
    q = Pair(4096)
    keys = (np.arange(16 * WG) % 32 + 1000).astype(np.int64)
    res = q.insert(keys)
    assert res.is_new.nonzero().flatten().tolist() == list(range(32)) and torch.equal(res.first.cpu(), torch.arange(16 * WG) % 32)
    assert (res.visits == 16 * WG // 32).all() and q.t.entries() == 32
    res = q.insert(keys[::-1].copy())                      # the smallest index of a key is now in the LAST workgroups
    assert not res.is_new.any() and (res.visits == 16 * WG // 16).all()


@pytest.mark.parametrize("capacity", [64, 4096])
def test_chains_that_share_a_home_and_wrap(capacity):
    last = keys_with_home(capacity, capacity - 1, 6)                          # one home, the table's last slot: the chain wraps
    mid = keys_with_home(capacity, 17, 3)
    p = Pair(capacity)
    res = p.insert(np.array(last[:4] + mid[:2], np.int64))
    assert sorted(res.entry[:4].tolist()) == [0, 1, 2, capacity - 1] and sorted(res.entry[4:].tolist()) == [17, 18]
    assert res.is_new.all()
    # a lookup must not stop early at the foreign keys of its chain; an absent key of the chain walks it to the empty slot behind
    found = p.lookup(np.array(last[:5] + mid + [last[3]], np.int64))
    assert found.entry[4].item() == -1 and found.entry[7].item() == -1 and (found.entry[:4] >= 0).all()
    res = p.insert(np.array([last[4], mid[2], last[0]], np.int64))            # new keys join behind their chains
    assert res.entry[:2].tolist() == [3, 19] and res.is_new.tolist() == [True, True, False]


def test_a_lookup_stops_at_the_first_empty_slot():
    """A table made by hand that BREAKS the invariant: a key one slot behind an empty home.  The lookup answers "absent", which shows
    that it stops at the empty slot; an insert places the key at its home, and from then on everybody finds it there."""
    capacity = 64
    k = keys_with_home(capacity, 9, 1)[0]
    t = KeyTable(capacity, DEV)
    state = t.state_dict()
    state["keys"][10] = k
    state["visits"][10] = 5
    t.load_state_dict(state)
    assert t.lookup(on_device([k]), visits=True).entry.tolist() == [-1]
    other = keys_with_home(capacity, 10, 1)[0]
    assert t.lookup(on_device([other])).entry.tolist() == [-1]                # (a foreign key in its home, then an empty slot)
    res = t.insert(on_device([k]), visits=True)
    assert res.entry.tolist() == [9] and res.is_new.tolist() == [True] and res.visits.tolist() == [1]
    assert t.lookup(on_device([k])).entry.tolist() == [9]


def test_special_keys_and_clear():
    p = Pair(64)
    res = p.insert(np.array([0, 1, 1, 0, TOP, -1, TOP + 1], np.int64))
    assert res.entry[0] == res.entry[1] == res.entry[2] == res.entry[3] and res.visits[:4].tolist() == [4] * 4 and p.t.entries() == 4
    assert res.is_new.tolist() == [True, False, False, False, True, True, True] and int(p.t.keys[res.entry[0]]) == 1
    assert p.lookup(np.array([1, 0, TOP, 2], np.int64)).entry[3].item() == -1
    res = p.insert(np.array([0, 5], np.int64), count=False)                   # MGX_KEY_NO_COUNT leaves the counts alone
    assert res.visits.tolist() == [4, 0] and res.is_new.tolist() == [False, True]
    p.t.clear()
    torch.cuda.synchronize()
    assert p.t.entries() == 0 and p.t.occupied().numel() == 0 and not p.t._buf.any()
    fresh = Pair(64, table=p.t)                                               # the cleared table is an empty table: epochs start anew
    res = fresh.insert(np.array([1, 9, 9], np.int64))
    assert res.is_new.tolist() == [True, True, False] and res.visits.tolist() == [1, 2, 2] and int(p.t.ctrl[1]) == 1
    fresh.lookup(np.array([TOP, 9], np.int64))
    state = p.t.state_dict()
    other = KeyTable(64, DEV)
    other.load_state_dict(state)
    twin = Pair(64, table=other)
    twin.m, twin.known = fresh.m, fresh.known
    twin.insert(np.array([9, 4], np.int64))


def test_full_tables():
    r = np.random.default_rng(7)
    keys = r.permutation(np.arange(1000, 1096, dtype=np.int64))
    p = Pair(64)
    p.insert(keys[:64])                                                       # filled exactly: no drop
    assert p.t.entries() == 64 and p.t.dropped() == 0 and p.t.occupied().numel() == 64
    res = p.insert(np.concatenate([keys[60:70], keys[:4], keys[64:66]]))      # deterministic: every new key is dropped, the old found
    assert (res.entry[4:10] == -1).all() and (res.entry[14:] == -1).all() and (res.entry[:4] >= 0).all() and p.t.dropped() == 8
    with pytest.raises(ValueError, match=r"KeyTable: 8 inserted key\(s\) were dropped"):
        p.t.check_errors()
    p.m.dropped = 0
    p.lookup(keys)
    # 96 distinct keys into an empty table of 64 in one call: WHICH 64 are placed is arrival order
    q = KeyTable(64, DEV)
    res = q.insert(on_device(keys), first=True, visits=True)
    placed = (res.entry >= 0).cpu().numpy()
    assert placed.sum() == 64 and q.entries() == 64 and q.dropped() == 32
    assert sorted(res.entry.cpu().numpy()[placed].tolist()) == list(range(64))
    assert res.is_new.cpu().numpy().tolist() == placed.tolist() and res.visits.cpu().numpy().tolist() == placed.astype(int).tolist()
    assert res.first.cpu().numpy().tolist() == np.where(placed, np.arange(96), -1).tolist()
    found = q.lookup(on_device(keys), visits=True)
    assert torch.equal(found.entry, res.entry) and torch.equal(found.visits, res.visits)        # dropped keys look up as -1
    assert q.keys[res.entry[res.entry >= 0]].cpu().tolist() == keys[placed].tolist()
    with pytest.raises(ValueError, match=r"KeyTable: 32 inserted key\(s\) were dropped.*capacity 64, 64 entries"):
        q.check_errors()
    q.check_errors()                                                          # raises once


# ---- real envs ---------------------------------------------------------------------------------------------------------------------

EMPTY8 = EnvSpec(8, 8, 2, 7, max_steps=8)


def test_a_captured_insert_is_a_new_call_at_every_replay():
    """state_key(out=keys), insert(keys, out=res) and lookup in one graph, replayed three times on envs that do not move: the first
    replay reports the new keys, the second and third none, and visits rises by one per replay -- the epoch lives in device memory."""
    from tests.test_env_snapshot import make_env
    from tests.test_episode_stats import actions_for
    B = 130
    env = make_env("pool", B=B, spec=EMPTY8, dev=DEV)
    for a in actions_for(B, 2, 3, 2).to(DEV):
        env.step(a, auto_reset=True)
    table = env.key_table(512)
    keys = torch.zeros(B, dtype=torch.int64, device=DEV)
    cur = torch.cuda.current_stream(torch.device(DEV))
    side, graph = torch.cuda.Stream(torch.device(DEV)), torch.cuda.CUDAGraph()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        env.state_key(out=keys)                                               # (everything bound and allocated before the capture)
        res = table.insert(keys, first=True, visits=True)
        found = table.lookup(keys, visits=True)
        table.clear()
        with torch.cuda.graph(graph, stream=side):
            env.state_key(out=keys)
            table.insert(keys, first=True, visits=True, out=res)
            table.lookup(keys, visits=True, out=found)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    assert table.entries() == 0 and int(table.ctrl[1]) == 0
    m = ModelTable(512)
    for replay in range(3):
        for o in (*res, *found):
            o.zero_()
        keys.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _, is_new, first, visits = m.insert(keys.cpu().numpy())
        assert res.is_new.cpu().numpy().tolist() == is_new.tolist() and bool(is_new.any()) == (replay == 0), replay
        assert res.first.cpu().numpy().tolist() == first.tolist() and res.visits.cpu().numpy().tolist() == visits.tolist(), replay
        assert torch.equal(found.entry, res.entry) and torch.equal(found.visits, res.visits)
        once = res.visits.clone() if replay == 0 else once                    # how often a key occurs in the call
        assert torch.equal(res.visits, (replay + 1) * once) and int(once.sum()) >= B              # one more visit per index and replay
        assert int(table.ctrl[1]) == replay + 1 and table.entries() == m.entries and table.dropped() == 0
    assert 1 < m.entries <= B
    env.check_errors()


def test_tables_of_an_env_against_its_oracle_twins():
    """venv.key_table() on a small real env, step by step against the table of an oracle-backed twin (the model launcher): state
    keys, a snapshot's keys into the same table, and obs_key()'s [B, A] shape"""
    from tests.test_env_snapshot import make_env
    from tests.test_episode_stats import actions_for
    from tests.test_state_key import KeyOracle

    class Oracle(KeyOracle, KeyTableModel):
        pass
    B, T = 130, 6
    env, twin = make_env("pool", B=B, spec=EMPTY8, dev=DEV), make_env("pool", B=B, spec=EMPTY8, backend=Oracle(EMPTY8))
    tables = [(env.key_table(1024), env.key_table(4096)), (twin.key_table(1024), twin.key_table(4096))]
    assert tables[0][0].device == env.agents.device and tables[0][0].backend is env.backend
    acts = actions_for(B, 2, T, 4)

    def same(got, want):
        assert got.entry.shape == want.entry.shape
        for g, w in zip(got[1:], want[1:]):
            assert g.cpu().tolist() == w.tolist()
        assert len(set(zip(got.entry.cpu().view(-1).tolist(), want.entry.view(-1).tolist()))) == len(set(want.entry.view(-1).tolist()))
    snaps = None
    for t in range(T):
        same(*[tb[0].insert(e.state_key(), first=True, visits=True) for e, tb in zip((env, twin), tables)])
        if t == 2:
            snaps = [e.snapshot() for e in (env, twin)]
        if t == 4:
            rows = torch.tensor([5, 129, 5, 0])
            same(*[tb[0].insert(s.state_key(rows.to(e.agents.device)), first=True, visits=True)
                   for s, e, tb in zip(snaps, (env, twin), tables)])
        env.step(acts[t].to(DEV), auto_reset=True)
        twin.step(acts[t], auto_reset=True)
        got, want = [tb[1].insert(e.obs_key(), first=True, visits=True) for e, tb in zip((env, twin), tables)]
        assert tuple(got.entry.shape) == (B, 2) and got.is_new.dtype is torch.bool
        same(got, want)
    for k in (0, 1):
        assert tables[0][k].entries() == tables[1][k].entries() > 8 and tables[0][k].dropped() == 0
    env.check_errors()


def test_the_example_searches_with_a_table():
    """examples/table_search.py with check=True at C2's batch, one root, depth 12: at every level the table chose what the torch
    formulation chooses, and nothing was dropped"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "table_search.py")
    mod_spec = importlib.util.spec_from_file_location("table_search", path)
    mod = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(mod)
    out = mod.run("c2", roots=1, depth=12, device=DEV, check=True)
    assert out["batch"] == 4096 and out["checked"] and out["drops"] == 0 and out["depth"] == 12 and not out["found"]
    assert len(out["new_per_level"]) == 12 and min(out["new_per_level"]) > 0 and out["table_entries"] == 1 + sum(out["new_per_level"])
